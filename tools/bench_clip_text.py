"""Once-per-step cost of the CLIP text tower on the GPU: K = 12 rank prompts (11 tokens each) through a seeded ViT-B text tower
(512 wide / 8 heads / 12 blocks / 77 positions / 512 outputs) -- this package's ``CLIPPromptEncoder`` on the prompts' compact rows
(with and without the shared prefix) against ``transformers``' ``CLIPModel`` text path on the same device and the same weights, in
fp32 and in bf16, over all 12 x 77 positions.  The claim under test is "fewer rows, same kernels", nothing more.

    python tools/bench_clip_text.py [--out FILE] [--calls N] [--repeats R]

Forward = text features under ``no_grad``.  Forward + backward = features, then the gradient back to the token embeddings (the HIP
tower: d prompts_embedding; HuggingFace: everything frozen but ``token_embedding.weight``, so its backward is the same chain of
input gradients plus an embedding scatter).  Host clock around N calls that end in a device synchronise, R windows per variant,
the variants ALTERNATING inside a round; reported: the median window and the spread, in us per call.  Needs the device (no fall-back)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import clip_text_cases as CC  # noqa: E402
import clip_text_helpers as CH  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_clip_text: no GPU (a timing taken anywhere else says nothing)")
import gc; gc.collect(); gc.freeze()   # noqa: E401,E702  torch's imported objects out of the collector's way (profiles/README.md)

CC.TOWERS["vitb"] = dict(width=512, heads=8, layers=12, vocab=CC.VOCAB, ctx=CC.CTX, out_dim=512)
SEED, K = 9201, 12
table, ctx_key, rank_keys = CC.prompt_table(SEED, 4)
W = CC.make_clip_weights("vitb", SEED)
tok = CC.ReplayTokenizer(table, CC.BOS, CC.EOS, CC.PAD, length=CC.CTX)
E = torch.nn.Embedding.from_pretrained(W["token_embedding.weight"].clone(), freeze=True)
from vlsa_amd.prompt_learner import RankPromptLearner  # noqa: E402
pl = RankPromptLearner(text_config=dict(max_num_tokens=CC.CTX, embedding_dim=512, embedding_dtype=torch.float32), tokenizer=tok,
                       token_embedding=E, num_base_ranks=4, num_ranks=K, num_tokens_per_rank=4, num_context_tokens=8,
                       rank_tokens_position="tail", init_context=ctx_key, init_rank_names=rank_keys).cuda()
enc = CH.clip_encoder("vitb", SEED)
for p in enc.parameters():
    p.requires_grad_(False)
enc = enc.cuda().eval()
pseudo = pl.pseudo_sentence_tokens
n_tok = int(pseudo.argmax(dim=-1)[0]) + 1

# HuggingFace: the same tensors under its names; token ids of sentences as long as the learner's
ids = torch.full((K, CC.CTX), CC.PAD, dtype=torch.long)
for i in range(K):
    body = [CC.BOS] + table[ctx_key] + (table[rank_keys[i % 4]] + [3] * 4)[:4] + [table["X."][1], CC.EOS]
    ids[i, :len(body)] = torch.tensor(body)
assert int(ids.argmax(dim=-1)[0]) + 1 == n_tok
ids, mask = ids.cuda(), (ids != CC.PAD).long().cuda()
hf = {}
for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    m = CH.hf_model("vitb", SEED).to(dtype).cuda().eval()
    for k, p in m.named_parameters():
        p.requires_grad_(k == "text_model.embeddings.token_embedding.weight")
    hf[name] = m


def hip_fwd(prefix):
    def run():
        with torch.no_grad():
            return enc(prompts_embedding=pl(), prompts_pseudo_tokens=pseudo, shared_prefix_len=prefix)
    return run


def hip_fwd_bwd(prefix):
    def run():
        pl.zero_grad(set_to_none=True)
        enc(prompts_embedding=pl(), prompts_pseudo_tokens=pseudo, shared_prefix_len=prefix).sum().backward()
    return run


def hf_features(m):
    out = m.get_text_features(input_ids=ids, attention_mask=mask)
    return getattr(out, "pooler_output", out)


def hf_fwd(m):
    def run():
        with torch.no_grad():
            return hf_features(m)
    return run


def hf_fwd_bwd(m):
    def run():
        m.zero_grad(set_to_none=True)
        hf_features(m).float().sum().backward()
    return run


L = pl.shared_prefix_len
variants = [("HIP tower, shared prefix", hip_fwd(L), hip_fwd_bwd(L)), ("HIP tower, row per position", hip_fwd(0), hip_fwd_bwd(0)),
            ("transformers CLIPModel fp32", hf_fwd(hf["fp32"]), hf_fwd_bwd(hf["fp32"])),
            ("transformers CLIPModel bf16", hf_fwd(hf["bf16"]), hf_fwd_bwd(hf["bf16"]))]
# same token ids, same weights: the two sides compute the same features
with torch.no_grad():
    a, b = enc(prompts_text=ids), hf_fwd(hf["fp32"])()
agree = (a - b.float()).abs().max().item()


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


times = {(name, which): [] for name, *_ in variants for which in ("forward", "forward + backward")}
for name, f, fb in variants:                     # every shape once, before any timed window
    window(f, 20), window(fb, 20)
for _ in range(args.repeats):
    for name, f, fb in variants:
        times[name, "forward"].append(window(f, args.calls))
        times[name, "forward + backward"].append(window(fb, args.calls))

rows_prefix, rows_plain = enc._plan(pseudo, ids.device, L).M, enc._plan(pseudo, ids.device, 0).M
lines = [f"CLIP ViT-B text tower (512 / 8 heads / 12 blocks / 77 positions / 512 outputs, seeded weights), K = {K} rank prompts of {n_tok} tokens",
         f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.repeats} windows of {args.calls} calls per variant, alternating; us per call",
         f"rows evaluated: HIP {rows_prefix} (shared prefix of {L} positions) / {rows_plain} (row per position); transformers {K * CC.CTX} (every position)",
         f"HIP features vs transformers fp32 on the same token ids: max|diff| {agree:.2e}", "",
         f"{'variant':32s} {'pass':20s} {'median':>9s} {'min':>9s} {'max':>9s}"]
for (name, which), t in times.items():
    lines.append(f"{name:32s} {which:20s} {statistics.median(t):9.1f} {min(t):9.1f} {max(t):9.1f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")

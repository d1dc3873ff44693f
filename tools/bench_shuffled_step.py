"""The optimizer step under a sampler that reshuffles every epoch (the reference's DataLoader(shuffle=True), runner/base_handler.py:241):
`python tools/bench_shuffled_step.py [--runs 5] [--epochs 2] [--out FILE]`.

Workload: bench.py's `train_step` leg -- its model (ordinal rank prompt learner through the frozen CONCH-size text tower, VLFAN with P = 12
TaskRes queries, IF-MLE + EMD, fused Adam) and its TCGA-like size mix (2k - 12k patches) -- over a RESIDENT bf16 set of 320 bags, 32 per
step, a fresh permutation per epoch (10 steps).  Three legs, each with a model of its own, interleaved run by run on one GPU:
  A  step(source.take(idx), t_all[idx], e_all[idx]): what a reshuffled epoch costs without the slots -- no batch repeats, always eager;
  B  set_epoch(...) / step_next(): the slots -- one graph serves every batch (set_epoch's upload and its one sync are inside the time);
  C  step(bags, t, e) on ONE fixed batch: the existing replay, a reference point (per-batch `groups`, no gather launch).
A run = `--epochs` epochs per leg; wall ms per step from HIP events around the run, host ms per step from the host clock around the same
calls (the host returns before the GPU is done).  Reported: every run's figures, the median per leg, and the spread (max - min) of the
runs.  The last line is the same as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import torch  # noqa: E402

M, BATCH, P, D, KT = 320, 32, 12, 512, 12


def build(device, graph, seed=1100):
    """bench.py train_step_leg's model and optimizer"""
    import text_cases as TC
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.prompt_adapter import PromptAdapter
    from vlsa_amd.prompt_encoder import CONCHPromptEncoder
    from vlsa_amd.prompt_learner import RankPromptLearner
    from vlsa_amd.train_step import TrainStep
    from vlsa_amd.vlsa import VLSA
    c = TC.TOWERS["conch"]
    enc = CONCHPromptEncoder(width=c["width"], heads=c["heads"], layers=c["layers"], vocab_size=c["vocab"], output_dim=c["out_dim"])
    enc.load_state_dict(TC.make_tower_weights("conch", 9001))
    for p_ in enc.parameters():
        p_.requires_grad_(False)
    table, ctx_key, names = TC.synthetic_prompt_table(c["vocab"], 9001, n_ctx=8)
    learner = RankPromptLearner(dict(max_num_tokens=127, embedding_dim=c["width"], embedding_dtype=torch.float32), TC.ReplayTokenizer(table),
                                enc.token_embedding, num_base_ranks=4, num_ranks=KT, num_tokens_per_rank=4, num_context_tokens=8,
                                init_context=ctx_key, init_rank_names=names)
    g = torch.Generator().manual_seed(seed)
    qnet = PromptAdapter(method="TaskRes", num_prompts=P, pretrained_prompt_features=torch.randn(P, D, generator=g), res_ratio=0.5)
    cfg = dict(name="VLFAN", dim_in=D, use_feat_proj=False, num_query=P, query="Text", query_pooling="mean", pred_head="default")
    net = VLSA.from_modules(cfg, prompt_learner=learner, prompt_encoder=enc, query_network=qnet).to(device).train()
    with torch.no_grad():
        qnet.residual_features.copy_(0.02 * torch.randn(P, D, generator=g))
    ps = [net.mil_encoder.Q.residual_features, net.mil_encoder.visual_adapter.weight, net.mil_encoder.visual_adapter.bias,
          learner.context_embeds, learner.rank_embeds, net.logit_scale]
    groups = [{"params": [p_ for p_ in ps if p_.dim() < 2], "weight_decay": 0.0}, {"params": [p_ for p_ in ps if p_.dim() >= 2], "weight_decay": 1e-5}]
    return TrainStep(net, SurvObjective(), FusedAdam(groups, lr=2e-4), graph=graph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2, help="epochs per run and leg")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.runs >= 3
    from vlsa_amd.functional import BagSet
    device = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    sizes = [int(x) for x in torch.randint(2000, 12000, (M,), generator=g)]
    gd = torch.Generator(device=device).manual_seed(1100)
    source = BagSet([torch.randn(n, D, device=device, generator=gd).to(torch.bfloat16) for n in sizes])
    t_all = torch.randint(0, KT, (M,), generator=g)
    e_all = (torch.rand(M, generator=g) < 0.45).float()
    e_all[t_all == KT - 1] = 1.0
    t_all, e_all = t_all.to(device), e_all.to(device)
    fixed = (source.take(range(BATCH)), t_all[:BATCH].clone(), e_all[:BATCH].clone())
    steps_per_epoch = M // BATCH
    ts = {"A": build(device, False), "B": build(device, True), "C": build(device, True)}

    def epoch(leg, perm):
        if leg == "A":
            perm_dev = perm.to(device)
            host = perm.tolist()
            for i in range(0, M, BATCH):
                idx = perm_dev[i:i + BATCH]
                ts["A"].step(source.take(host[i:i + BATCH]), t_all[idx], e_all[idx])
        elif leg == "B":
            t0 = time.perf_counter()
            ts["B"].set_epoch(source, t_all, e_all, perm, BATCH)
            in_set_epoch.append((time.perf_counter() - t0) * 1e3)
            for _ in range(steps_per_epoch):
                ts["B"].step_next()
        else:
            for _ in range(steps_per_epoch):
                ts["C"].step(*fixed)

    in_set_epoch = []
    gp = torch.Generator().manual_seed(7)
    for _ in range(2):                                   # warm-up: allocator pools, the captures of B and C
        perm = torch.randperm(M, generator=gp)
        for leg in "ABC":
            epoch(leg, perm)
    torch.cuda.synchronize()
    del in_set_epoch[:]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall, host = {k: [] for k in "ABC"}, {k: [] for k in "ABC"}
    for r in range(a.runs):
        perms = [torch.randperm(M, generator=gp) for _ in range(a.epochs)]
        for leg in ("ABC", "BCA", "CAB")[r % 3]:         # interleaved, the order rotating
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for perm in perms:
                epoch(leg, perm)
            h = time.perf_counter() - t0
            e1.record()
            torch.cuda.synchronize()
            n = a.epochs * steps_per_epoch
            wall[leg].append(e0.elapsed_time(e1) / n)
            host[leg].append(h / n * 1e3)
    ts["B"].check_epoch()
    how = {k: v.describe() for k, v in ts.items()}
    slots = ts["B"].epoch_state()["full"]
    names = {"A": "A  step(source.take(idx), ...): eager, per-batch groups", "B": "B  set_epoch / step_next: slots, one graph",
             "C": "C  step() on one fixed batch: the existing replay"}
    lines = [f"reshuffled optimizer step: {M} resident bf16 bags of 2k-12k patches ({sum(sizes)} patches), {BATCH} per step, "
             f"{steps_per_epoch} steps per epoch, a fresh permutation per epoch; {a.runs} runs x {a.epochs} epochs per leg, interleaved",
             f"{torch.cuda.get_device_name(0)}; B's fixed groups = {slots.groups()}, C's groups = {fixed[0].groups()}",
             f"{'leg':58s} {'wall ms/step: median':>20s} {'spread':>8s} {'host ms/step: median':>21s} {'spread':>8s}"]
    res = {}
    for k in "ABC":
        w, h = wall[k], host[k]
        res[k] = {"wall_ms_per_step": {"median": statistics.median(w), "spread": max(w) - min(w), "runs": w},
                  "host_ms_per_step": {"median": statistics.median(h), "spread": max(h) - min(h), "runs": h}, "how": how[k]}
        lines.append(f"{names[k]:58s} {statistics.median(w):20.3f} {max(w) - min(w):8.3f} {statistics.median(h):21.3f} {max(h) - min(h):8.3f}")
    for k in "ABC":
        lines.append(f"{k} runs, wall ms/step: " + " ".join(f"{x:.3f}" for x in wall[k]) + "   host ms/step: " + " ".join(f"{x:.3f}" for x in host[k]))
    for k in "ABC":
        lines.append(f"{k}: {how[k]}")
    # B's host time is the step_next calls plus, once per epoch, set_epoch: the order's upload and the ONE sync that reads the status
    # word -- the host waits there for the GPU to finish the epoch it has queued (it runs ahead of the GPU by the whole epoch)
    se = statistics.median(in_set_epoch)
    b_steps = statistics.median(host["B"]) - se / steps_per_epoch
    res["B"]["host_ms_set_epoch_per_epoch"] = se
    res["B"]["host_ms_per_step_without_set_epoch"] = b_steps
    lines.append(f"B host: set_epoch {se:.3f} ms per epoch (median; upload + the one sync, which waits for the queued epoch), "
                 f"step_next alone {b_steps:.3f} ms per step")
    spread = max(res[k]["wall_ms_per_step"]["spread"] for k in "ABC")
    d_ba = res["B"]["wall_ms_per_step"]["median"] - res["A"]["wall_ms_per_step"]["median"]
    d_bc = res["B"]["wall_ms_per_step"]["median"] - res["C"]["wall_ms_per_step"]["median"]
    lines.append(f"B - A = {d_ba:+.3f} ms per step, B - C = {d_bc:+.3f} ms per step (largest spread of a leg's runs: {spread:.3f} ms)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"shuffled_step": res, "B_minus_A_ms": d_ba, "B_minus_C_ms": d_bc, "largest_spread_ms": spread}))


if __name__ == "__main__":
    main()

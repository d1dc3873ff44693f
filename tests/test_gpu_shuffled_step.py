"""TrainStep.set_epoch / step_next: the optimizer step over batches a reshuffling sampler draws (reference: DataLoader(shuffle=True),
runner/base_handler.py:241).  The bags stay in one resident BagSet; ``vlsa_batch_gather`` copies each step's descriptor rows and labels
into slots at fixed addresses (``functional.BagSlots``), so ONE hipGraph per batch size serves every batch.  Checked here: replayed slot
steps are the eager slot steps, the eager slot steps follow the trajectory of ``step(source.take(idx), ...)``, the slots hold exactly the
picked rows after every step, models outside the size-agnostic set stay eager, and the gather launch on its own refuses what it must.

The fixtures are those of test_gpu_train_step_graph.py (same seeded model, K = P = 12); every comparison prints its figure first."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cases
import text_cases as TC

pytestmark = pytest.mark.gpu

K, TOWER, TSEED = 12, "train", 9300
M, BATCH, EPOCHS = 10, 4, 4
# every boundary the streaming kernels branch on (one row, below / at a 64-row unit, past a 256-row tile, several tiles, several
# workgroups per bag) and nothing larger
SIZES = [1, 17, 64, 257, 600, 1500, 33, 128, 900, 1201]


def _deepmil():
    """test_gpu_deepmil_train_batch's VLSA over a DeepMIL encoder (gated attention over the patches; dropout off: one trajectory)"""
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=False, drop_rate=0.0, pooling="gated_attention",
               pred_head="default")
    torch.manual_seed(11)
    net = VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=cases.LOGIT_SCALE).cuda().train()
    return net, [p for p in net.parameters() if p.requires_grad]


def _model(num_query=12, feat_proj=False):
    """test_gpu_train_step_graph._model.  Outside the size-agnostic set: num_query = 13 on bf16 bags (the backward for more than 12
    queries sizes its partial sums on the host, by the batch's largest bag) and feat_proj (a trainable Feat_Projecter in front: its
    output, and the chunk plan kept on the bag set, are sized by the batch's total rows)"""
    from vlsa_amd.prompt_adapter import PromptAdapter
    from vlsa_amd.prompt_encoder import CONCHPromptEncoder
    from vlsa_amd.prompt_learner import RankPromptLearner
    from vlsa_amd.vlsa import VLSA
    P = num_query
    torch.manual_seed(12)                                  # (the Feat_Projecter's own initialisation)
    params = cases.make_params(P, K, 9201)
    c = TC.TOWERS[TOWER]
    enc = CONCHPromptEncoder(width=c["width"], heads=c["heads"], layers=c["layers"], vocab_size=c["vocab"], output_dim=c["out_dim"])
    enc.load_state_dict(TC.make_tower_weights(TOWER, TSEED))
    for p_ in enc.parameters():
        p_.requires_grad_(False)
    table, ctx_key, names = TC.synthetic_prompt_table(c["vocab"], TSEED)
    pl = RankPromptLearner(dict(max_num_tokens=127, embedding_dim=c["width"], embedding_dtype=torch.float32), TC.ReplayTokenizer(table),
                           enc.token_embedding, num_base_ranks=4, num_ranks=K, num_tokens_per_rank=4, num_context_tokens=8,
                           init_context=ctx_key, init_rank_names=names)
    qnet = PromptAdapter(method="TaskRes", num_prompts=P, pretrained_prompt_features=params["prompt"], res_ratio=0.5)
    cfg = dict(name="VLFAN", dim_in=512, use_feat_proj=feat_proj, num_query=P, query="Text", query_pooling="mean", pred_head="default")
    net = VLSA.from_modules(cfg, prompt_learner=pl, prompt_encoder=enc, query_network=qnet, logit_scale_init=cases.LOGIT_SCALE).cuda().train()
    with torch.no_grad():
        qnet.residual_features.copy_(params["resid"])
        net.mil_encoder.visual_adapter.weight.copy_(params["W"])
        net.mil_encoder.visual_adapter.bias.copy_(params["b"])
    named = [net.mil_encoder.Q.residual_features, net.mil_encoder.visual_adapter.weight, net.mil_encoder.visual_adapter.bias,
             pl.context_embeds, pl.rank_embeds, net.logit_scale]
    if feat_proj:
        named += [p_ for p_ in net.mil_encoder.feat_proj.parameters() if p_.requires_grad]
    return net, named


def _groups(ps):
    return [{"params": [p for p in ps if p.dim() < 2], "weight_decay": 0.0}, {"params": [p for p in ps if p.dim() >= 2], "weight_decay": 1e-5}]


KINDS = {"vlfan12": lambda: _model(12), "vlfan13": lambda: _model(13), "featproj": lambda: _model(12, True), "deepmil": _deepmil}


@functools.lru_cache(maxsize=None)
def _source(dtype, kind="vlfan12"):
    from vlsa_amd.functional import BagSet
    g = torch.Generator().manual_seed(78)
    bags = [cases.make_bag(n, 9700 + i, "clustered").to(dtype).cuda() for i, n in enumerate(SIZES)]
    t_all = torch.randint(0, (K if kind != "deepmil" else 4) - 1, (M,), generator=g).cuda()      # (the DeepMIL model has 4 bins)
    e_all = (torch.rand(M, generator=g) < 0.5).float().cuda()
    return BagSet(bags), t_all, e_all


def _orders():
    g = torch.Generator().manual_seed(79)
    return [torch.randperm(M, generator=g).numpy() for _ in range(EPOCHS)]


def _pick(x, idx):
    return x[torch.as_tensor(np.asarray(idx), device=x.device)]


def _batches(order):
    return [order[i:i + BATCH] for i in range(0, len(order), BATCH)]


def _stepper(graph, kind):
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    net, named = KINDS[kind]()
    return net, named, TrainStep(net, SurvObjective(), FusedAdam(_groups(named), lr=1e-3), graph=graph)


@functools.lru_cache(maxsize=None)
def _run_slots(graph, dtype, kind="vlfan12", groups=None):
    """the 12 steps through set_epoch / step_next.  After every step: the slots against the source (bit-equal), the cursor against the
    rows consumed, the parameters' version counters, and a read of the current text features (between the steps, replays included)."""
    source, t_all, e_all = _source(dtype, kind)
    net, named, ts = _stepper(graph, kind)
    losses, text, consumed, ptrs = [], [], 0, {}
    for order in _orders():
        ts.set_epoch(source, t_all, e_all, order, BATCH, groups=groups)
        consumed = 0
        for idx in _batches(order):
            v0 = [p._version for p in named]
            losses.append(float(ts.step_next()))
            assert all(p._version > v for p, v in zip(named, v0)), len(losses)
            consumed += len(idx)
            st = ts.epoch_state()
            slots = st["full"] if len(idx) == BATCH else st["tail"]
            here = (slots.desc().data_ptr(), slots.t.data_ptr(), slots.e.data_ptr())
            assert ptrs.setdefault(len(idx), here) == here and len(slots) == len(idx)        # fixed addresses
            assert np.array_equal(slots.desc().cpu().numpy(), source.rows[idx]), (len(losses), idx)
            assert torch.equal(slots.t, _pick(t_all, idx)) and torch.equal(slots.e, _pick(e_all, idx)), (len(losses), idx)
            assert int(st["cursor"]) == consumed and int(st["status"]) == 0
            if kind == "vlfan12":
                net.eval()
                with torch.no_grad():
                    text.append(net.forward_text_only().clone())
                net.train()
        with pytest.raises(StopIteration):
            ts.step_next()
    d = ts.describe()
    ts.close()                                               # (reads the last epoch's status word)
    return losses, [p.detach().clone() for p in named], text, d


@functools.lru_cache(maxsize=None)
def _run_api(dtype, kind="vlfan12"):
    """the same order through the existing API: TrainStep(graph=False).step(source.take(idx), t_all[idx], e_all[idx])"""
    source, t_all, e_all = _source(dtype, kind)
    _, named, ts = _stepper(False, kind)
    losses = []
    for order in _orders():
        for idx in _batches(order):
            losses.append(float(ts.step(source.take(idx), _pick(t_all, idx), _pick(e_all, idx))))
    return losses, [p.detach().clone() for p in named]


def _agree(tag, run_a, run_b, tol):
    la, pa = run_a[0], run_a[1]
    lb, pb = run_b[0], run_b[1]
    assert len(la) == len(lb) == EPOCHS * 3
    dl = max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(la, lb))
    dp = max((a - b).abs().max().item() / max(1.0, a.abs().max().item()) for a, b in zip(pa, pb))
    print(f"{tag}: losses of the first epoch {[round(x, 6) for x in la[:3]]} / {[round(x, 6) for x in lb[:3]]}")
    print(f"{tag}: losses {dl:.2e}, parameters {dp:.2e} (relative to max(1, |x|); bound {tol:.0e})")
    assert dl <= tol, (tag, la, lb)
    assert dp <= tol, tag


def _captured(d):
    assert d["captures"] == 2 and d["why_eager"] is None, d
    assert d["slot_replays"]["full"] >= 5 and d["slot_replays"]["tail"] >= 1, d


def test_replayed_slot_steps_equal_the_eager_slot_steps():
    """same kernels, same `groups`: the bound the project holds between replayed and eager steps"""
    g, e = _run_slots(True, torch.bfloat16), _run_slots(False, torch.bfloat16)
    _captured(g[3])
    assert e[3]["captures"] == 0 and e[3]["replays"] == 0 and e[3]["eager_steps"] == EPOCHS * 3, e[3]
    _agree("slots: graph against eager (bf16)", e, g, 5e-6)


def test_eager_slot_steps_follow_the_existing_api():
    """`groups` is one value per slots object but chosen per batch by step(): another row partition, the project's bound for that"""
    _agree("slots eager against step(source.take(idx)) (bf16)", _run_api(torch.bfloat16), _run_slots(False, torch.bfloat16), 1e-4)


def test_fp32_source():
    g, e = _run_slots(True, torch.float32), _run_slots(False, torch.float32)
    _captured(g[3])
    _agree("slots: graph against eager (fp32)", e, g, 5e-6)


@pytest.mark.parametrize("kind,why", [("vlfan13", "12 queries"), ("deepmil", "DeepMIL"), ("featproj", "Feat_Projecter")])
def test_a_model_outside_the_size_agnostic_set_stays_eager(kind, why):
    """13 queries on bf16 bags: the backward sizes its partial sums by the largest bag of the batch, on the host.  A DeepMIL encoder and
    a VLFAN behind a Feat_Projecter: their chunk plans (row offsets, tile tables, buffer sizes, kept on the bag set) are built from the
    batch's sizes -- the slots must drop them on every refill, or the next batch runs on the previous batch's tables."""
    losses, params, _, d = _run_slots(True, torch.bfloat16, kind)
    assert d["captures"] == 0 and d["replays"] == 0 and d["eager_steps"] == EPOCHS * 3, d
    assert d["why_eager"] and why in d["why_eager"], d
    _agree(f"{kind}: slots (eager) against step(source.take(idx))", _run_api(torch.bfloat16, kind), (losses, params), 1e-4)


def test_a_fixed_groups_other_than_the_batches_own():
    """set_epoch(groups=): a value the batches would not choose, i.e. another split of the rows into partial sums than step() takes"""
    from vlsa_amd.functional import BagSlots, choose_groups
    source, _, _ = _source(torch.bfloat16)
    default = BagSlots(source, BATCH).groups()
    own = {choose_groups([SIZES[i] for i in idx], 0) for order in _orders() for idx in _batches(order) if len(idx) == BATCH}
    forced = next(g for g in (1, 2, 4) if g != default and g not in own)
    print(f"groups: the slots' default {default}, the full batches' own {sorted(own)}, forced {forced}")
    g, e = _run_slots(True, torch.bfloat16, "vlfan12", forced), _run_slots(False, torch.bfloat16, "vlfan12", forced)
    _captured(g[3])
    _agree(f"groups = {forced}: graph against eager", e, g, 5e-6)
    _agree(f"groups = {forced}: slots eager against step(source.take(idx))", _run_api(torch.bfloat16), e, 1e-4)


def test_replays_move_the_version_counters_and_the_text_cache():
    """(the counters are asserted after every step inside the run) forward_text_only() between the steps sees the current prompts"""
    tg, te = _run_slots(True, torch.bfloat16)[2], _run_slots(False, torch.bfloat16)[2]
    assert len(tg) == len(te) == EPOCHS * 3
    for a, b in zip(te, tg):
        assert (a - b).abs().max().item() < 1e-5
    assert not torch.equal(tg[9], tg[10])                   # read after two consecutive full-size replays: not served from a cache
    assert (tg[4] - tg[10]).abs().max().item() > 1e-4       # ... and over six replayed steps the prompts did move


# ---- the gather launch through ctypes alone: no case here reaches a streaming kernel (the descriptor rows are made-up words) ----
def _gather_fixture(Mg, B, order, cursor):
    g = torch.Generator().manual_seed(80)
    f = {"src": torch.randint(-2 ** 62, 2 ** 62, (Mg, 3), generator=g).cuda(), "t_all": torch.randint(0, 99, (Mg,), generator=g).cuda(),
         "e_all": torch.rand(Mg, generator=g).cuda(), "order": torch.tensor(order, dtype=torch.int64).cuda(),
         "cursor": torch.tensor([cursor], dtype=torch.int64).cuda(), "desc": torch.full((B, 3), -7, dtype=torch.int64).cuda(),
         "t": torch.full((B,), -7, dtype=torch.int64).cuda(), "e": torch.full((B,), -7.0).cuda(),
         "status": torch.zeros(1, dtype=torch.int32).cuda()}
    return f


def _gather(f, Mg, B, L=None):
    from vlsa_amd import _native
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    code = _native.load().vlsa_batch_gather(p(f["src"]), p(f["t_all"]), p(f["e_all"]), Mg, p(f["order"]), len(f["order"]) if L is None else L,
                                            B, p(f["cursor"]), p(f["desc"]), p(f["t"]), p(f["e"]), p(f["status"]),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


def _untouched(f, cursor):
    return (int(f["cursor"]) == cursor and bool((f["desc"] == -7).all()) and bool((f["t"] == -7).all()) and bool((f["e"] == -7.0).all()))


@pytest.mark.parametrize("B,Mg", [(1, 3), (5, 7), (64, 64), (64, 200)])
def test_gather_copies_rows_and_labels_and_moves_the_cursor(B, Mg):
    g = torch.Generator().manual_seed(81 + B + Mg)
    order = torch.randint(0, Mg, (2 * B + 3,), generator=g).tolist()
    f = _gather_fixture(Mg, B, order, 0)
    for k in range(2):
        assert _gather(f, Mg, B) == 0
        idx = f["order"][k * B:(k + 1) * B]
        assert int(f["cursor"]) == (k + 1) * B and int(f["status"]) == 0
        assert torch.equal(f["desc"], f["src"][idx]) and torch.equal(f["t"], f["t_all"][idx]) and torch.equal(f["e"], f["e_all"][idx])
    # the third batch would overrun L = 2 B + 3 only when B > 3: the cursor check refuses it, the second batch stays
    kept = [x.clone() for x in (f["desc"], f["t"], f["e"])]
    assert _gather(f, Mg, B) == 0
    if B > 3:
        from vlsa_amd import _native
        assert int(f["status"]) == _native.GATHER_BAD_CURSOR and int(f["cursor"]) == 2 * B
        assert all(torch.equal(a, b) for a, b in zip(kept, (f["desc"], f["t"], f["e"])))
    else:
        assert int(f["status"]) == 0 and int(f["cursor"]) == 3 * B


@pytest.mark.parametrize("bad,at", [(7, 0), (7, 3), (10 ** 12, 2), (-1, 0), (-1, 3), (-2 ** 40, 1)])
def test_gather_refuses_an_index_outside_the_source(bad, at):
    from vlsa_amd import _native
    Mg, B = 7, 4
    order = [1, 6, 0, 3, 2, 5, 4, 1]
    order[4 + at] = bad                                   # in the SECOND batch
    f = _gather_fixture(Mg, B, order, 4)
    assert _gather(f, Mg, B) == 0
    assert int(f["status"]) == _native.GATHER_BAD_INDEX and _untouched(f, 4)


@pytest.mark.parametrize("cursor,L", [(6, 8), (8, 8), (5, 8), (-1, 8), (-4, 8), (2 ** 62, 8), (0, 3), (0, 0)])
def test_gather_refuses_a_cursor_outside_the_order(cursor, L):
    from vlsa_amd import _native
    Mg, B = 7, 4
    f = _gather_fixture(Mg, B, [1, 6, 0, 3, 2, 5, 4, 1], cursor)
    assert _gather(f, Mg, B, L=L) == 0
    assert int(f["status"]) == _native.GATHER_BAD_CURSOR and _untouched(f, cursor)


def test_gather_refuses_bad_arguments_on_the_host():
    from vlsa_amd import _native
    f = _gather_fixture(7, 4, [0, 1, 2, 3], 0)
    for Mg, B, L in ((7, 0, 4), (7, 65, 4), (0, 4, 4), (7, 4, -1)):
        assert _gather(f, Mg, B, L=L) == _native.EINVAL
    assert int(f["status"]) == 0 and _untouched(f, 0)


def test_set_epoch_reports_a_refused_gather_of_the_epoch_that_ended():
    """the one host sync per epoch: a status word left behind by a gather launch raises at the next set_epoch"""
    from vlsa_amd import VlsaNativeError, _native
    source, t_all, e_all = _source(torch.bfloat16)
    _, _, ts = _stepper(False, "vlfan12")
    order = _orders()[0]
    ts.set_epoch(source, t_all, e_all, order, BATCH)
    ts.step_next()
    ts.epoch_state()["status"].fill_(_native.GATHER_BAD_INDEX)     # (what a launch that refused its picks leaves)
    with pytest.raises(VlsaNativeError):
        ts.set_epoch(source, t_all, e_all, order, BATCH)
    ts.set_epoch(source, t_all, e_all, order, BATCH)                # the word was cleared: the next epoch begins
    assert float(ts.step_next()) > 0.0


def test_bagslots_groups_and_refusals():
    from vlsa_amd.functional import BagSlots, choose_groups
    source, t_all, e_all = _source(torch.bfloat16)
    s = BagSlots(source, BATCH, t_all=t_all, e_all=e_all)
    assert np.array_equal(s.rows, source.rows[:BATCH])
    rep = sorted(SIZES)[::M // BATCH][:BATCH]
    assert s.groups() == s.groups(8) == choose_groups(rep, 0)
    assert s.chunk(0, BATCH) is s and s.chunk(0, 64) is s and s.sizes == tuple(SIZES[:BATCH])
    assert np.array_equal(s.desc().cpu().numpy(), source.rows[:BATCH]) and torch.equal(s.t, t_all[:BATCH]) and torch.equal(s.e, e_all[:BATCH])
    d0 = s.desc().data_ptr()
    s.follow([9, 2, 5, 0])
    assert s.sizes == (SIZES[9], SIZES[2], SIZES[5], SIZES[0]) and s[1] is source[2] and s.desc().data_ptr() == d0 and s.groups() == choose_groups(rep, 0)
    assert BagSlots(source, BATCH, groups=2).groups() == 2
    for kw in (dict(groups=3), dict(groups=8), dict(t_all=t_all[:5]), dict(e_all=e_all.cpu()), dict(t_all=t_all.float())):
        with pytest.raises(ValueError):
            BagSlots(source, BATCH, **kw)
    with pytest.raises(ValueError):
        BagSlots(list(source), BATCH)
    with pytest.raises(ValueError):
        BagSlots(source, M + 1)

"""MIL encoders usable as ``VLSA.mil_encoder`` -- drop-in counterparts of the reference's ``model/deepmil.py``
classes (same constructor kwargs, attribute names and state-dict keys), with the N-sized arithmetic in HIP.

    VLFAN         model/deepmil.py:74-215     language-guided cross-attention aggregation (the shipped encoder)
    FeatMIL       model/deepmil.py:40-67      mean / max / identity (zero-shot)
    DeepMIL       model/deepmil.py:222-292    ABMIL-style (gated-)attention pooling over the N patches
    DSMIL         model/deepmil.py:638-721    dual-stream MIL (instance max + critical-instance attention), an SA baseline
    logit_pooling model/deepmil.py:16-37      top-k / mean pooling of per-patch class logits

The reference picks the encoder with ``getattr(model.deepmil, cfg['name'])(**cfg)`` (model/utils_vl.py:129-138);
``vlsa_amd.vlsa.build_mil_encoder`` does the same lookup in this module.
"""
from __future__ import annotations

import collections
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as VF
from .layers import Adapter, Attention_Pooling, Feat_Projecter, Gated_Attention_Pooling

__all__ = ["logit_pooling", "FeatMIL", "VLFAN", "DeepMIL", "DSMIL"]


_LOGIT_POOLINGS = {"logit_mean": None, "logit_max": 1}


def _parse_logit_pooling(method: str):
    """'logit_mean' -> None (all patches), 'logit_max' -> 1, 'logit_top<k>' -> k; anything else is not a logit pooling."""
    if method in _LOGIT_POOLINGS:
        return _LOGIT_POOLINGS[method]
    head, _, digits = method.partition("logit_top")
    if head == "" and digits.isdigit():
        return int(digits)
    raise NotImplementedError(f"The pooling ({method}) is not implemented.")


def logit_pooling(logits: torch.Tensor, method: str):
    """logits: [N, C] per-patch class logits -> (preds[1], pooled[1, C]).  (model/deepmil.py:16-37)
    The per-class top-k mean runs in HIP; when the logits carry a gradient (zero-shot prompt tuning) the selection is
    done with torch.topk so that autograd reaches them, as in the reference."""
    topk = _parse_logit_pooling(method)
    N = logits.size(0)
    k = N if topk is None else min(topk, N)
    if torch.is_grad_enabled() and logits.requires_grad:
        pooled = logits.topk(k, dim=0).values.mean(dim=0, keepdim=True) if k < N else logits.mean(dim=0, keepdim=True)
    else:
        pooled = VF.topk_mean(logits.t().contiguous(), k)[None, :]
    return pooled.argmax(dim=1), pooled


class FeatMIL(nn.Module):
    """Feature aggregation only: 'mean' | 'max' over the patches, anything else = identity (zero-shot)."""

    def __init__(self, pooling="mean", **kwargs):
        super().__init__()
        self.network = nn.Identity()
        self.pooling = pooling

    def forward(self, X):
        assert X.shape[0] == 1
        if self.pooling == "mean":
            return VF.scored_pool(X, None)[None, :]
        if self.pooling == "max":
            return VF.colmax(X)[None, :]
        return X.squeeze(0)


class VLFAN(VF.nat.TransientCaches, nn.Module):
    """Language-guided visual feature aggregation network (model/deepmil.py:74-215).

    P query vectors (text prototypes through a query network, or an ``nn.Parameter``) cross-attend over the N
    patches with cosine scores x 100, softmax over the patches; the P aggregated rows are pooled over the queries
    and passed through the visual adapter.  The cross attention runs in the HIP streaming kernels.
    """

    _transient = {"_step_query": None, "_enc_plans": None, "_fused_scores": None, "_coattn_scale": None}

    def __init__(self, dim_in=1024, dim_hid=256, use_feat_proj=True, drop_rate=0.25, query="Parameter", num_query=10,
                 gated_query=False, query_pooling="mean", pred_head="default", dim_reduction=4, keep_ratio=0.8, **kwargs):
        super().__init__()
        self._pos_gated_query = -1
        self.feat_proj = Feat_Projecter(dim_in, dim_in) if use_feat_proj else None
        self.num_query = num_query
        self.query_type = query
        self.gated_query = gated_query
        assert self.query_type in ["Parameter", "Text"]
        if self.query_type != "Parameter":
            self.Q = None  # call reset_query() with the query network
        else:
            self.Q = nn.Parameter(torch.randn(num_query + 1 if gated_query else num_query, dim_in))
        assert query_pooling in ["mean", "max", "weight", "attention", "gated_attention"]
        if query_pooling == "attention":
            self.query_pooling = Attention_Pooling(dim_in, dim_hid)
        elif query_pooling == "gated_attention":
            self.query_pooling = Gated_Attention_Pooling(dim_in, dim_hid, dropout=drop_rate)
        elif query_pooling == "weight":
            self.query_pooling = nn.Parameter(torch.randn(1, num_query))
        else:
            self.query_pooling = query_pooling
        self.pred_head = pred_head
        self.visual_adapter = nn.Identity() if pred_head == "Identity" else nn.Linear(dim_in, dim_in)
        self.use_custom_coattn = True
        self.coattn_logit_scale = torch.ones([]) * math.log(100)  # plain tensor attribute, as in the reference

    # -- reference API ---------------------------------------------------------------------------------
    def get_coattn_logit_scale(self):
        return self.coattn_logit_scale.exp()

    def coattn_scale(self) -> float:
        """exp(coattn_logit_scale) as a Python float, cached per (tensor object, in-place version): the per-bag routes ask for it
        once per bag."""
        t = self.coattn_logit_scale
        c = self.__dict__.get("_coattn_scale")
        if c is None or c[0] is not t or c[1] != t._version:
            c = self.__dict__["_coattn_scale"] = (t, t._version, float(t.detach().exp()))
        return c[2]

    def reset_query(self, query_network):
        assert self.query_type != "Parameter", f"Cannot override Q (query) for query_type ({self.query_type})."
        self.Q = query_network

    def get_query(self):
        assert self.Q is not None, f"You have to call `reset_query` to reset query for query_type ({self.query_type})."
        return self.Q() if callable(self.Q) else self.Q

    def step_query(self):
        """``get_query()`` for the per-bag training path: when the queries come from a module (the text PromptAdapter), its
        output -- WITH its autograd graph -- is shared by all bags that see the same parameter versions, train / eval flag and
        grad mode (the reference's step evaluates the adapter once per bag: runner/vlsa_handler.py:267-269; same values, 32 x
        the launches and autograd nodes).  A backward pass through the cached tensor frees that graph: the next call rebuilds.
        NOT shared when the query network is stochastic: an active ``nn.Dropout`` (the 'FC' PromptAdapter has Dropout(0.25),
        model/prompt_learners/prompt_adapter.py:95-104) draws a fresh mask per bag in the reference, so every call evaluates
        the network again -- a cached output would give all bags of a step (a frozen adapter: of the whole run) one mask."""
        Qs = self.Q
        if not isinstance(Qs, nn.Module):
            return self.get_query()
        key = [torch.is_grad_enabled()]
        stack = [Qs]
        while stack:
            m = stack.pop()
            if m.training and isinstance(m, nn.modules.dropout._DropoutNd) and m.p > 0:
                self._step_query = None
                return self.get_query()
            key.append((id(m), m.training))
            for t in m._parameters.values():
                if t is not None:
                    key.append((id(t), t._version, t.requires_grad))
            for t in m._buffers.values():
                if t is not None:
                    key.append((id(t), t._version))
            stack.extend(c for c in m._modules.values() if c is not None)
        key = tuple(key)
        cached = getattr(self, "_step_query", None)
        if cached is None or cached[0] != key:
            q = self.get_query()
            if q.requires_grad and q.grad_fn is not None:
                q.register_hook(self._drop_step_query)
            cached = self._step_query = (key, q)
        return cached[1]

    def _drop_step_query(self, *_):
        self._step_query = None

    def query_div_loss(self, last_div=True, **kws):
        """Diversity penalty on the queries = mean |cosine| (model/deepmil.py:157-168): between the gate query (last row)
        and every other query when there is one and ``last_div``; otherwise over all ordered pairs of distinct queries."""
        unit = F.normalize(self.get_query(), dim=-1)
        n = unit.shape[0]
        if last_div and n == self.num_query + 1:
            cos = unit[:-1] @ unit[-1]                       # [P]: gate vs the P prototypes
            return cos.abs().mean()
        gram = (unit @ unit.t()).abs()
        off_diag = gram.sum() - gram.diagonal().sum()        # the diagonal (self-similarity) does not count
        return off_diag / (n * (n - 1))

    def forward_query_pooling(self, X):
        """[B, P, C] aggregated rows -> ([B, C] pooled, scores of the pooling module or None)  (model/deepmil.py:133-150)"""
        pool = self.query_pooling
        if isinstance(pool, nn.Module):                       # Attention_Pooling / Gated_Attention_Pooling over the P rows
            needs_graph = torch.is_grad_enabled() and (X.requires_grad or any(p.requires_grad for p in pool.parameters()))
            dropout_on = pool.training and isinstance(pool, Gated_Attention_Pooling) and pool.fc1[2].p > 0
            if X.is_cuda and not needs_graph and not dropout_on and X.shape[1] <= 16 and X.shape[2] <= 1024:
                return VF.query_pool_attention(X, pool)       # inference: two HIP launches instead of ~10 torch ops on [P, 512]
            return pool(X)
        if isinstance(pool, nn.Parameter):                    # 'weight': learnable convex combination of the P rows
            mix = torch.softmax(pool, dim=-1)                 # [1, P]
            return torch.einsum("op,bpc->bc", mix, X), None
        if pool == "mean":
            return X.mean(dim=1), None
        return X.amax(dim=1), None

    # -- fused inference support -------------------------------------------------------------------------
    def fused_head_spec(self):
        """(pool mode, pool weight, W, b) if pooling + adapter can run in the fused HIP head, else None.  A Feat_Projecter
        does not stand in the way: the inference routes project the bag first (``project``: one fused HIP launch per bag)."""
        if isinstance(self.query_pooling, str):
            mode, pw = self.query_pooling, None
        elif isinstance(self.query_pooling, nn.Parameter):
            mode, pw = "weight", self.query_pooling
        elif not (self.query_pooling.training and isinstance(self.query_pooling, Gated_Attention_Pooling) and self.query_pooling.fc1[2].p > 0):
            mode, pw = "module", self.query_pooling       # (gated-)attention over the P rows: vlsa_query_pool_attention
        else:
            return None
        if isinstance(self.visual_adapter, nn.Linear):
            return mode, pw, self.visual_adapter.weight, self.visual_adapter.bias
        return mode, pw, None, None

    def project(self, X):
        """The bag as the cross attention sees it: Feat_Projecter(X) when use_feat_proj=True (model/deepmil.py:176-179)."""
        return X if self.feat_proj is None else self.feat_proj(X)

    def _projecter_trains(self) -> bool:
        return (self.feat_proj is not None and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.feat_proj.parameters()))

    def _fused_encode(self, X, ret_with_attn):
        """Inference, nothing to differentiate: the whole encoder (query preparation, streaming aggregation, merge, attention
        weights, query pooling, adapter) as ONE host call into the C ABI (``VlfanInferencePlan``; the text part of the fused
        head is fed a dummy class).  None when the configuration has no fused form."""
        spec = self.fused_head_spec()
        if (spec is None or spec[0] == "module" or torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
                or not X.is_cuda or X.shape[-1] != 512 or X.shape[1] == 0 or X.dtype not in (torch.float32, torch.bfloat16)):
            return None
        mode, pw, W, b = spec
        X2 = VF._bag2d(X)
        Q = self.get_query()
        if torch.is_grad_enabled() and Q.requires_grad:
            return None      # a query that needs a gradient but is no registered parameter (closure / plain callable): autograd route
        Q = Q.detach().float().contiguous()
        P = Q.shape[0] - (1 if self.gated_query else 0)
        if not (1 <= P <= 16):
            return None
        N, dev = X2.shape[0], X2.device
        plans = self.__dict__.setdefault("_enc_plans", {})
        key = (N, dev, bool(ret_with_attn), P, mode, W is None)
        plan = plans.get(key)
        if plan is None:
            if len(plans) > 32:
                plans.clear()
            plan = plans[key] = VF.VlfanInferencePlan(N, 512, P, 1, dev, gated=self.gated_query, pool=mode, identity_head=W is None,
                                                      want_attn=ret_with_attn, coattn_scale=self.coattn_scale())
            plan._dummy = (torch.ones(1, 512, device=dev), torch.zeros((), device=dev))
        outs = {"v": torch.empty(512, dtype=torch.float32, device=dev)}
        if ret_with_attn:
            outs["A"] = torch.empty(P, N, dtype=torch.float32, device=dev)
        plan.run(X2, Q, plan._dummy[0], plan._dummy[1], None if W is None else W.detach().float().contiguous(),
                 None if b is None else b.detach().float().contiguous(),
                 None if pw is None else pw.detach().float().reshape(-1).contiguous(), outs=outs)
        v = outs["v"][None]
        return (v, outs["A"][None]) if ret_with_attn else v

    def forward(self, X, ret_with_attn=False):
        assert X.shape[0] == 1
        if self.feat_proj is not None:
            X = self.feat_proj(X)
        if not (torch.is_grad_enabled() and X.requires_grad):
            fused = self._fused_encode(X, ret_with_attn)
            if fused is not None:
                return fused
        Q = self.get_query()
        if self.gated_query:
            assert self._pos_gated_query == -1, "The gated query is placed at the end by default."
            assert Q.shape[0] == self.num_query + 1, f"Query number is expected to be {self.num_query + 1}."
        scale = self.coattn_scale()
        # HIP forward and backward: dQ always, dX as well when the bag carries a gradient (a trainable Feat_Projecter in front:
        # its output is an fp32 [N, 512] bag; vlsa_vlfan_backward_dx)
        out, A = VF.vlfan_cross_attention(X, Q, gated=self.gated_query, coattn_scale=scale, want_attn=ret_with_attn)
        pooled_out, pooled_ext = self.forward_query_pooling(out.unsqueeze(0))
        visual_features = self.visual_adapter(pooled_out)
        if ret_with_attn:
            A = A.unsqueeze(0)
            attn = (A, pooled_ext.detach()) if pooled_ext is not None else A
            return visual_features, attn
        return visual_features

    def forward_bags(self, bags, ret_with_attn=False, projected=False):
        """Differentiable forward over a list of bags (each [1, N_i, C] or [N_i, C]) sharing this encoder: the cross
        attention of all bags runs in the persistent multi-bag kernels (forward and backward), the P x C tail as batched
        torch ops.  Equals ``torch.cat([self(x) for x in bags])``; one training step of the reference
        (runner/vlsa_handler.py:260-289) is 32 such bags.  Returns visual features [B, C]; with ``ret_with_attn`` also the
        per-bag attention exactly as ``forward(x, ret_with_attn=True)`` hands it out: a list of ``A`` [1, P, N_i], or of
        ``(A, pool_scores)`` when the query pooling is a module (model/deepmil.py:206-215).  ``projected``: the bags already
        went through ``project``."""
        if self.feat_proj is not None and not projected:
            # one fused HIP launch per chunk of 64 bags, fp32 out; a projecter that trains records its LayerNorm statistics and
            # receives its gradient from the HIP backward kernels (the aggregation hands dX back for the projected bags)
            bags = self.feat_proj.forward_bags(bags)
        outs_cat, attn = self._aggregate_bags(bags, ret_with_attn)
        pooled_out, pooled_ext = self.forward_query_pooling(outs_cat)
        feats = self.visual_adapter(pooled_out)
        if not ret_with_attn:
            return feats
        if pooled_ext is not None:
            attn = [(a, pooled_ext[i:i + 1].detach()) for i, a in enumerate(attn)]
        return feats, attn

    def aggregate_bags(self, bags):
        """The P aggregated rows of every bag, [B, P, C], differentiable w.r.t. the queries (persistent multi-bag kernels forward
        and backward) -- ``forward_bags`` without the query pooling and the adapter.  A trainable Feat_Projecter is part of
        the graph (HIP forward + backward; the aggregation hands dX back for the projected fp32 bags)."""
        if self.feat_proj is not None:
            bags = self.feat_proj.forward_bags(bags)
        return self._aggregate_bags(bags, False)[0]

    def _aggregate_bags(self, bags, ret_with_attn):
        Q = self.get_query()
        scale = self.coattn_scale()
        outs, attn = [], []
        for chunk in VF.bag_chunks(bags):           # (a BagSet's sub-sets stay BagSets: checked once, descriptor rows kept)
            r = VF.vlfan_cross_attention_bags(chunk, Q, gated=self.gated_query, coattn_scale=scale, want_attn=ret_with_attn)
            if ret_with_attn:
                outs.append(r[0])
                attn.extend(a.unsqueeze(0) for a in r[1])
            else:
                outs.append(r)
        return VF.cat(outs), attn


def pool_mean_max(flat, mode: str, bag_grad: bool = False, join=VF.cat) -> torch.Tensor:
    """'mean' / 'max' pooling [B, C] of a list of [N_i, C] bags, for DeepMIL and FeatMIL (model/deepmil.py:57-60,271-274 per bag).
    Bags the batched kernels take (``uniform_bags``): VF.mean_pool_bags / VF.max_pool_bags per <= 64 bags -- under a bag gradient one
    autograd node per chunk -- except ONE bag's max without a gradient, which is the single-bag launch pair's.  Anything else bag by
    bag: torch ops under a bag gradient and on CPU tensors, the single-bag launch pair otherwise.  bag_grad: the caller differentiates
    through the bags (``forward_bags``; the routes without autograd say no).  join: what makes one tensor of the chunks' results."""
    if VF.uniform_bags(flat) and (mode == "mean" or bag_grad or len(flat) > 1):
        pool = VF.mean_pool_bags if mode == "mean" else VF.max_pool_bags
        return join([pool(chunk) for chunk in VF.bag_chunks(flat)])
    if mode == "mean":
        return torch.stack([x.float().mean(dim=0) if (bag_grad or not x.is_cuda) else VF.scored_pool(x, None) for x in flat])
    return torch.stack([x.float().amax(dim=0) if (bag_grad or not x.is_cuda) else VF.colmax(x) for x in flat])


def _device_bag(X2) -> bool:
    """one bag the fused score kernels read: bf16 or fp32 device rows, at least one"""
    return X2.is_cuda and X2.dtype in (torch.bfloat16, torch.float32) and X2.shape[0] > 0


class _DropoutSeed:
    """nn.Module mixin: the seed words of the batched training forwards whose dropout masks are drawn inside the kernels"""

    def _dropout_seed_word(self, device) -> torch.Tensor:
        """The seed of one batched training forward as a device word: a per-module device counter, its base drawn ONCE from torch's CPU
        generator (``torch.manual_seed`` governs it), advanced in-stream by every call -- eagerly and in a captured graph's replays
        alike -- and snapshotted, so that the backward of this call reads the seed its forward read."""
        ctr = self.__dict__.get("_drop_counter")
        if ctr is None or ctr.device != device:
            base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            ctr = self._drop_counter = torch.full((1,), base, dtype=torch.int64, device=device)
        ctr.add_(1)
        return ctr.clone()


# what DeepMIL's four routes read of its pooling module: gated; the three Linear layers; weights: the six tensors the kernels take;
# drop_p: the ACTIVE dropout rate (0.0 in eval and for the ungated module); rates_equal: both branches drop at one rate (the kernels
# draw one mask rate); widths_fused: 512 -> 256, the fused score kernels' sizes
_PoolSpec = collections.namedtuple("_PoolSpec", "gated lin_a lin_g lin_o weights drop_p rates_equal widths_fused")


class DeepMIL(VF.nat.TransientCaches, _DropoutSeed, nn.Module):
    """ABMIL-style encoder (model/deepmil.py:222-292): optional Feat_Projecter, mean / max / (gated-)attention pooling
    over the N patches, Adapter head mixed with ``keep_ratio`` or a Linear head."""

    _transient = {"_fused_scores": None}

    def __init__(self, dim_in=1024, dim_hid=256, num_cls=2, use_feat_proj=True, drop_rate=0.25, pooling="attention",
                 pred_head="default", dim_reduction=4, keep_ratio=0.8, **kwargs):
        super().__init__()
        assert pooling in ["mean", "max", "attention", "gated_attention"]
        assert pred_head in ["default", "Adapter"]
        self.feat_proj = Feat_Projecter(dim_in, dim_in) if use_feat_proj else None
        if pooling == "gated_attention":
            self.sigma = Gated_Attention_Pooling(dim_in, dim_hid, dropout=drop_rate)
        elif pooling == "attention":
            self.sigma = Attention_Pooling(dim_in, dim_hid)
        else:
            self.sigma = pooling
        self.pred_head = pred_head
        if pred_head == "Adapter":
            assert 0 <= keep_ratio <= 1.0
            self.keep_ratio = keep_ratio
            self.visual_adapter = Adapter(dim_in, dim_reduction)
        else:
            self.g = nn.Linear(dim_in, num_cls)

    def pool_bags(self, flat):
        """Pooled bag vectors [B, C] of a list of validated [N_i, 512] device bags (one dtype) without autograd: the
        (gated-)attention poolings run as ONE score launch and ONE pooling launch per <= 64 bags when the fused kernel applies
        (512 -> 256 hidden, no active dropout), otherwise bag by bag.  model/deepmil.py:270-283 per bag."""
        sg = self.sigma
        if isinstance(sg, str):
            if sg == "max":
                return pool_mean_max(flat, sg)
            # (this route's launches as tests/model_routes_expected.json pins them: a set's projected bags as a list -- table staged, not
            # derived by four torch launches -- and torch.cat over one chunk too, a copy; dropping either takes a recording of its own)
            return pool_mean_max(list(flat) if isinstance(flat, VF.ProjectedBags) else flat, sg, join=torch.cat)
        s = self._pool_spec()
        if s.widths_fused and s.drop_p == 0 and VF.uniform_bags(flat):        # no mask is drawn: the two rates need not agree
            return torch.cat([self._scores().pool_bags(chunk, *s.weights)[0] for chunk in VF.bag_chunks(flat)])
        return torch.stack([VF.scored_pool(x, self._attention_scores(x)) for x in flat])

    def _pool_spec(self) -> _PoolSpec:
        """the pooling module's parts, per call (plain dict look-ups: seven nn.Sequential.__getitem__ calls are 10 us of a 40 us module call)"""
        sg = self._modules["sigma"]
        sm = sg._modules
        if isinstance(sg, Gated_Attention_Pooling):
            f1, sc = sm["fc1"]._modules, sm["score"]._modules
            lin_a, lin_g, lin_o, p_a, p_g = f1["0"], sc["0"], sm["fc2"], f1["2"].p, sc["2"].p
            weights = (lin_a.weight, lin_a.bias, lin_g.weight, lin_g.bias, lin_o.weight, lin_o.bias)
            drop_p = float(p_a) if (sg.training and p_a > 0) else 0.0
        else:
            at = sm["attention"]._modules
            lin_a, lin_g, lin_o, p_a, p_g, drop_p = at["0"], None, at["2"], 0.0, 0.0, 0.0
            weights = (lin_a.weight, lin_a.bias, None, None, lin_o.weight, lin_o.bias)
        return _PoolSpec(lin_g is not None, lin_a, lin_g, lin_o, weights, drop_p, p_a == p_g,
                         lin_a.in_features == 512 and lin_a.out_features == 256)

    def _scores(self):
        """the fused score kernels' host object (packed weights, scratch), made on first use"""
        fs = self.__dict__.get("_fused_scores")
        if fs is None:
            fs = self._fused_scores = VF.FusedAttnScores()
        return fs

    def head(self, f):
        """[B, C] pooled bag vectors -> what the encoder returns (model/deepmil.py:283-288): the Adapter mixed in with ``keep_ratio``, or ``g``"""
        if self.pred_head == "Adapter":
            return self.keep_ratio * f + (1 - self.keep_ratio) * self.visual_adapter(f)
        return self.g(f)

    def _attention_scores(self, X2):
        """raw scores a[N] of the pooling module on all patches.  512 -> 256 hidden (the reference's sizes): ONE fused MFMA kernel,
        hidden activations in registers -- inference, and under autograd as well (HIP backward that recomputes them tile by tile,
        vlsa_attn_scores_backward), the gated module's training-mode dropout included (counter-based masks inside both kernels).
        Other widths, or a bag that itself carries a gradient: library GEMMs for the hidden projections + torch / HIP elementwise."""
        sg = self._modules["sigma"]
        s = self._pool_spec()
        lin_a, drop_p = s.lin_a, s.drop_p
        grad_mode = torch.is_grad_enabled()
        bag_grad = grad_mode and X2.requires_grad
        need_grad = bag_grad or (grad_mode and any(p.requires_grad for p in sg.parameters()))
        if not bag_grad and s.rates_equal and s.widths_fused and _device_bag(X2):
            if need_grad or drop_p > 0:
                return VF.attn_scores_autograd(X2, self._scores(), *s.weights, drop_p=drop_p)
            return self._scores()(X2, *s.weights)
        VF.nat.note_torch_route("DeepMIL attention scores", X2.shape[0],
                                f"widths {lin_a.in_features} -> {lin_a.out_features}, bag gradient {bag_grad}: the fused score kernel covers 512 -> 256 "
                                "hidden units, bags without a gradient of their own and equal dropout rates in both branches")
        Xf = X2 if X2.dtype == torch.float32 else X2.float()
        if isinstance(sg, Attention_Pooling):
            lin1, lin2 = sg.attention[0], sg.attention[2]
            H = Xf @ lin1.weight.t()
            if need_grad:
                return (torch.tanh(H + lin1.bias) @ lin2.weight.t() + lin2.bias).squeeze(-1)
            return VF.attn_scores(H, None, lin1.bias, None, lin2.weight, lin2.bias)
        la, lg, l2 = sg.fc1[0], sg.score[0], sg.fc2
        H, Hg = Xf @ la.weight.t(), Xf @ lg.weight.t()
        if need_grad or drop_p > 0:
            e = sg.fc1[2](torch.tanh(H + la.bias)) * sg.score[2](torch.sigmoid(Hg + lg.bias))
            return (e @ l2.weight.t() + l2.bias).squeeze(-1)
        return VF.attn_scores(H, Hg, la.bias, lg.bias, l2.weight, l2.bias)

    def forward_bags(self, bags, ret_with_attn=False, projected=False):
        """A list of bags (each [1, N_i, C] or [N_i, C]; a ``BagSet`` is taken as checked) through this encoder as a batch:
        ``torch.cat([self(x) for x in bags])`` up to fp32 rounding, with ``ret_with_attn`` also the per-bag attention as
        ``forward(x, ret_with_attn=True)`` hands it out (raw scores for Attention_Pooling, softmax weights for the gated module).
        (Gated) attention pooling with 512 -> 256 hidden units runs as one autograd node per <= 64 bags
        (VF.attn_pool_bags_autograd: three launches forward, one backward pass + reductions, dropout seeds from a device counter);
        mean / max pooling as batched launches -- under a bag gradient (a trainable projecter in front) as one node per <= 64 bags
        (VF.mean_pool_bags / VF.max_pool_bags: the row gradients of all bags in one launch), and max pooling behind a trainable
        projecter that this call runs itself as projecter + max in one node over the selected rows (VF.project_max_pool_bags).  The
        batched max follows the reference's ``torch.max``: where a column's maximum is tied, its gradient goes to the first maximal
        row (the per-bag ``forward`` splits it, ``amax``).  ``projected``: the bags already went through ``feat_proj``."""
        flat = bags if isinstance(bags, VF.BagSet) else [VF._bag2d(x) for x in bags]
        sg = self.sigma
        f = None
        if (sg == "max" and self.feat_proj is not None and not projected and self.feat_proj.trains()
                and self.feat_proj.serves_batch(flat)):
            # a trainable projecter in front of the max: projecter and pooling as one node that keeps the selected rows only
            f = self.feat_proj.max_pool_bags(flat)
        elif self.feat_proj is not None and not projected:
            flat = self.feat_proj.forward_bags(flat)          # fp32 [N, 512]; a trainable projecter gets dX from the pooling
        if len(flat) == 0:
            raise ValueError("forward_bags needs at least one bag")
        attn = None
        if f is not None:
            pass
        elif isinstance(sg, str):
            f = pool_mean_max(flat, sg, bag_grad=torch.is_grad_enabled() and any(x.requires_grad for x in flat))
        else:
            s = self._pool_spec()
            if not (s.widths_fused and s.rates_equal and VF.uniform_bags(flat)):     # (the kernels draw both branches' masks at ONE rate)
                outs = [self.forward(x[None], ret_with_attn=ret_with_attn, _projected=True) for x in flat]     # other widths: per bag
                if ret_with_attn:
                    return torch.cat([o[0] for o in outs]), [o[1] for o in outs]
                return torch.cat(outs)
            feats, scores = [], []
            for chunk in VF.bag_chunks(flat):
                seed = self._dropout_seed_word(chunk[0].device) if s.drop_p else None
                pooled, a = VF.attn_pool_bags_autograd(chunk, self._scores(), *s.weights, drop_p=s.drop_p, seed_word=seed)
                feats.append(pooled)
                if ret_with_attn:
                    o = 0
                    for x in chunk:
                        n = x.shape[0]
                        scores.append(a[o:o + n])
                        o += n
            f = VF.cat(feats)
            if ret_with_attn:
                attn = [(a[None, :] if not s.gated else F.softmax(a, dim=0)[None, :]).detach() for a in scores]
        logit = self.head(f)
        if ret_with_attn:
            if attn is None:
                raise NotImplementedError("ret_with_attn: mean / max pooling has no attention (model/deepmil.py:270-283)")
            return logit, attn
        return logit

    def forward(self, X, ret_with_attn=False, _projected=False):
        assert X.shape[0] == 1
        if self.feat_proj is not None and not _projected:
            X = self.feat_proj(X)
        raw_attn = fused_logit = None
        x_grad = torch.is_grad_enabled() and X.requires_grad   # a trainable Feat_Projecter in front: the pooling must hand dX back
        module = self._modules.get("sigma")     # (one dict read; None: 'mean' / 'max', a plain attribute)
        if module is None and self.sigma == "mean":
            out_feat = X.float().mean(dim=1) if x_grad else VF.scored_pool(X, None)[None, :]
        elif module is None:
            out_feat = X.float().amax(dim=1) if x_grad else VF.colmax(X)[None, :]
        else:
            X2 = VF._bag2d(X)
            s = self._pool_spec()
            fits = s.widths_fused and _device_bag(X2)
            if x_grad and fits and s.rates_equal:
                # scores + pooling as ONE autograd node whose backward is HIP end to end: parameter gradients AND
                # dX = dHa Wa + dHg Wg + A dpooled (vlsa_attn_scores_backward_dx); 512 -> 256 hidden, the reference's sizes
                pooled, a = VF.attn_pool_autograd(X2, self._scores(), *s.weights, drop_p=s.drop_p)
                out_feat = pooled[None, :]
            else:
                fused = None
                if not torch.is_grad_enabled() and fits and s.drop_p == 0:       # no mask is drawn: the two rates need not agree
                    # inference on a large bf16 bag: scores and pooling in ONE launch (vlsa_gated_scores_pool / _adapter)
                    adapter = None
                    if self.pred_head == "Adapter":
                        fc = self.visual_adapter._modules["fc"]._modules
                        W1, W2 = fc["0"].weight, fc["2"].weight
                        if W1.shape[1] == 512 and W2.shape[0] == 512 and W1.shape[0] % 4 == 0:
                            adapter = (W1, W2, self.keep_ratio)
                    fused = self._scores().scores_and_pool(X2, *s.weights, adapter=adapter)
                if fused is not None:
                    out_feat, a = fused[0], fused[1]
                    if len(fused) == 3:
                        fused_logit = fused[2]
                else:
                    a = self._attention_scores(X2)
                    if x_grad:         # other layer widths than 512 -> 256: library GEMMs (see _attention_scores) + torch pooling
                        out_feat = torch.softmax(a, dim=0)[None, :] @ X2.float()
                    else:
                        out_feat = VF.scored_pool(X2, a)[None, :]
            if ret_with_attn:  # what the reference hands back: raw scores (attention) / softmax weights (gated attention)
                raw_attn = a[None, :] if not s.gated else F.softmax(a, dim=0)[None, :]
        if fused_logit is not None:
            logit = fused_logit                      # (computed behind the pooling in the same host call)
        elif (self.pred_head == "Adapter" and out_feat.is_cuda
              and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.visual_adapter.fc.parameters()))):
            fc = self.visual_adapter.fc
            logit = VF.adapter_head(out_feat, fc[0].weight, fc[2].weight, self.keep_ratio)[None, :]   # two small HIP launches
        else:
            logit = self.head(out_feat)
        if ret_with_attn:
            return logit, raw_attn.detach()
        return logit


class _FCLayer(nn.Module):
    """model/deepmil.py:638-644: holds ``fc.0`` (the instance classifier).  Parameters only: DSMIL.forward drives the kernels."""

    def __init__(self, in_size, out_size=1):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(in_size, out_size))


class _BClassifier(nn.Module):
    """model/deepmil.py:661-671: holds ``q``, ``v.0`` (dropout) / ``v.1`` and ``fcc``.  Parameters only."""

    def __init__(self, input_size, hid_size, output_class, dropout_v=0.0):
        super().__init__()
        self.q = nn.Linear(input_size, hid_size)
        self.v = nn.Sequential(nn.Dropout(dropout_v), nn.Linear(input_size, hid_size))
        self.fcc = nn.Conv1d(output_class, output_class, kernel_size=hid_size)


class DSMIL(VF.nat.TransientCaches, _DropoutSeed, nn.Module):
    """DSMIL (Li et al., CVPR 2021; model/deepmil.py:692-721) with the reference's constructor and state-dict keys
    (``i_classifier.fc.0.*``, ``b_classifier.q.*``, ``b_classifier.v.1.*``, ``b_classifier.fcc.*``, ``feat_proj.*``).

    The reference projects all N rows through ``q`` and ``v``; here the module runs as two streaming passes over the bag with the
    ``num_cls`` class rows as queries (csrc/dsmil.hip: instance maxima, critical rows, online-softmax aggregation, head), forward
    and backward in HIP, for ``dim_in = 512``, ``dim_hid = 256``, ``num_cls <= 16``.  Gradients reach the eight DSMIL parameters;
    the bag rows get none, so a ``Feat_Projecter`` in front must be frozen while DSMIL trains.  Equal instance scores resolve to the
    lowest row index (the reference's ``torch.sort`` leaves ties open)."""

    _transient = {}

    def __init__(self, dim_in=1024, dim_hid=256, num_cls=2, use_feat_proj=True, drop_rate=0.25, **kwargs):
        super().__init__()
        self.feat_proj = Feat_Projecter(dim_in, dim_in) if use_feat_proj else None
        self.i_classifier = _FCLayer(in_size=dim_in, out_size=num_cls)
        self.b_classifier = _BClassifier(dim_in, dim_hid, num_cls, dropout_v=drop_rate)

    def _weights(self):
        bc = self.b_classifier._modules
        fc = self.i_classifier._modules["fc"]._modules["0"]
        q, v, fcc = bc["q"], bc["v"]._modules["1"], bc["fcc"]
        return fc.weight, fc.bias, q.weight, q.bias, v.weight, v.bias, fcc.weight, fcc.bias

    def forward_bags(self, bags, ret_with_attn=False, projected=False, ret_critical=False):
        """A list of bags (each [1, N_i, 512] or [N_i, 512]; a ``BagSet`` is taken as checked) as batches of <= 64 per launch chain:
        ``torch.cat([self(x) for x in bags])`` bit for bit.  Returns logits [B, C]; with ``ret_with_attn`` also the list of per-bag
        attention [1, N_i] (``A.mean(dim=1)`` of the reference); with ``ret_critical`` also the critical rows [B, C] (int32)."""
        Wc, bcl, Wq, bq, Wv, bv, Wf, bf = w = self._weights()
        if Wc.shape[1] != 512 or Wq.shape[0] != 256 or not (1 <= Wc.shape[0] <= 16):
            raise VF.VlsaNativeError(f"DSMIL: the HIP kernels cover dim_in = 512, dim_hid = 256, num_cls <= 16 (got {Wc.shape[1]}, "
                                     f"{Wq.shape[0]}, {Wc.shape[0]}); there is no other route")
        grad, is_set = torch.is_grad_enabled(), isinstance(bags, VF.BagSet)
        if not is_set and len(bags) == 0:
            raise ValueError("forward_bags needs at least one bag")
        VF._need_gpu(*(() if is_set else bags))
        # (the three refusals in the order they always had: a bag's gradient, the projecter's, then the bags' shapes)
        if grad and any(x.requires_grad for x in bags):
            raise VF.VlsaNativeError("DSMIL: the bag requires grad, but the HIP backward produces parameter gradients only (no dX)")
        if self.feat_proj is not None and not projected:
            if grad and any(p.requires_grad for p in self.feat_proj.parameters()):
                raise VF.VlsaNativeError("DSMIL: a trainable Feat_Projecter needs the gradient of the bag rows, which the DSMIL backward does "
                                         "not produce; freeze feat_proj (requires_grad_(False)) or run under torch.no_grad()")
        if not is_set:
            bags = VF.checked_bags(bags, 512, "DSMIL takes non-empty bags with 512 features, one dtype (bf16 or fp32) and one device",
                                   non_empty=True)
        drop = self.b_classifier._modules["v"]._modules["0"]
        drop_p = float(drop.p) if (self.training and drop.p > 0) else 0.0
        logits, attn, crit = [], [], []
        for chunk in VF.bag_chunks(bags):
            if self.feat_proj is not None and not projected:
                chunk = self.feat_proj.forward_bags(chunk)
                if not isinstance(chunk, VF.ProjectedBags):
                    chunk = [VF._bag2d(x) for x in chunk]
            seed = self._dropout_seed_word(chunk[0].device) if drop_p else None
            lg, a, cr = VF.dsmil_bags(chunk, *w, drop_p=drop_p, seed_word=seed, want_attn=ret_with_attn)
            logits.append(lg)
            crit.append(cr)
            if ret_with_attn:
                attn.extend(t[None, :] for t in a.split([int(x.shape[0]) for x in chunk]))
        out = (VF.cat(logits),)
        if ret_with_attn:
            out += (attn,)
        if ret_critical:
            out += (VF.cat(crit),)
        return out[0] if len(out) == 1 else out

    def forward(self, X, **kwargs):
        assert X.shape[0] == 1
        ret_attn = bool(kwargs.get("ret_with_attn"))
        ret_crit = bool(kwargs.get("ret_critical"))
        res = self.forward_bags([X], ret_with_attn=ret_attn, ret_critical=ret_crit)
        if not (ret_attn or ret_crit):
            return res
        res = list(res)
        if ret_attn:
            res[1] = res[1][0]
        return tuple(res)


class DeepAttnMISL(nn.Module):
    """DeepAttnMISL (Yao et al., MedIA 2020; model/deepmil.py:542-580) with the reference's constructor and state-dict keys
    (``phis.0.*`` -- the 1x1 convolution, weight [256, 512, 1, 1] --, ``attention_net.0.*``, ``attention_net.3.{fc1.0, score.0, fc2}.*``,
    ``output_layer.*``).

    The reference gathers each cluster's rows, runs the convolution on them and pools; here ``phis`` and the per-cluster mean are ONE
    HIP streaming pass over the bag (csrc/cluster_pool.hip: the [N, 256] activations never reach memory; an empty cluster gives a
    zero row; an id outside [0, num_clusters) belongs to no cluster), forward and backward, for ``dim_in = 512``, ``dim_hid = 256``,
    ``num_clusters <= 16``.  Everything behind it is ``num_clusters`` rows per bag and stays torch modules, batched over
    [B, num_clusters, 256].  Gradients reach every parameter; the bag rows get none, and they must be finite.

    The tail is EVALUATED IN FLOAT64 (float64 copies of its fp32 parameters through ``functional_call``, autocast switched off around
    it; logits and gradients come back as fp32): the attention branch's gradients are differences of nearly equal cluster rows, 1e-7
    .. 1e-10 of the others, which fp32 resolves to about 2e-3 of their largest entry only.  It is ``num_clusters`` rows per bag, so
    the cost is a few small float64 launches; the modules, their dropout and their gradients are torch's own."""

    def __init__(self, dim_in=512, dim_hid=256, num_cls=1, num_clusters=8, dropout=0.25, **kwargs):
        super().__init__()
        self.dim_hid = dim_hid
        self.num_clusters = num_clusters
        self.phis = nn.Sequential(nn.Conv2d(dim_in, dim_hid, 1), nn.ReLU())
        self.pool1d = nn.AdaptiveAvgPool1d(1)
        self.attention_net = nn.Sequential(nn.Linear(dim_hid, dim_hid), nn.ReLU(), nn.Dropout(dropout),
                                           Gated_Attention_Pooling(dim_hid, dim_hid, dropout=dropout))
        self.output_layer = nn.Linear(in_features=dim_hid, out_features=num_cls)

    def cluster_features(self, bags, cluster_ids, ret_state=False):
        """h_cluster [B, num_clusters, 256] of a list of bags (each [1, N_i, 512] or [N_i, 512]) in chunks of <= 64 per launch chain;
        ret_state: also the cluster sizes [B, Kc] and the ReLU mask bits [sum N_i, 8] the backward reads"""
        conv = self.phis._modules["0"]
        Wp, bp, Kc = conv.weight, conv.bias, int(self.num_clusters)
        if tuple(Wp.shape) != (256, 512, 1, 1) or bp is None or not (1 <= Kc <= 16):
            raise VF.VlsaNativeError(f"DeepAttnMISL: the HIP kernels cover dim_in = 512, dim_hid = 256, num_clusters <= 16 (got "
                                     f"{Wp.shape[1]}, {Wp.shape[0]}, {Kc}); there is no other route")
        if len(bags) == 0 or len(bags) != len(cluster_ids):
            raise ValueError("forward_bags needs at least one bag and one cluster-id tensor per bag")
        out = [VF.cluster_pool_bags(chunk, ids, Wp, bp, num_clusters=Kc, ret_state=ret_state)
               for chunk, ids in zip(VF.bag_chunks(bags), VF.bag_chunks(cluster_ids))]
        return tuple(VF.cat(o) for o in zip(*out)) if ret_state else VF.cat(out)

    def forward_bags(self, bags, cluster_ids, ret_state=False):
        """logits [B, num_cls] of a list of bags and their cluster ids: ``torch.cat([self(x, c) for x, c in zip(bags, cluster_ids)])``"""
        hc = self.cluster_features(bags, cluster_ids, ret_state)
        state = hc[1:] if ret_state else ()
        hc = hc[0] if ret_state else hc
        # the tail in float64 (see the class docstring); autocast would take its products back down to 16 bits
        with torch.autocast(device_type=hc.device.type, enabled=False):
            tail = {k: p.double() for k, p in self.attention_net.named_parameters()}
            H, _ = torch.func.functional_call(self.attention_net, tail, (hc.double(),))          # [B, 256], [B, Kc]
            out = F.linear(H, self.output_layer.weight.double(), self.output_layer.bias.double()).to(hc.dtype)
        return (out, hc, *state) if ret_state else out

    def forward(self, X, cluster_id, *args):
        return self.forward_bags([X], [cluster_id])


# ---- ILRA (Xiang et al., ICLR 2023; model/deepmil.py:409-535) ---------------------------------------------------------------------
def _ilra_initialize_weights(model):
    """model/deepmil.py:409-417"""
    for m in model.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


class _IlraMHA(nn.Module):
    """The parameters of the reference's ``MultiHeadAttention`` block (model/deepmil.py:420-452) under its own names; it is never
    called: ``ILRA.forward_bags`` reads the parameters and drives the kernels."""

    def __init__(self, dim_Q, dim_K, dim_V, num_heads, ln=False, gated=False):
        super().__init__()
        self.dim_V, self.num_heads = dim_V, num_heads
        self.multihead_attn = nn.MultiheadAttention(dim_V, num_heads)
        self.fc_q = nn.Linear(dim_Q, dim_V)
        self.fc_k = nn.Linear(dim_K, dim_V)
        self.fc_v = nn.Linear(dim_K, dim_V)
        if ln:
            self.ln0 = nn.LayerNorm(dim_V)
            self.ln1 = nn.LayerNorm(dim_V)
        self.fc_o = nn.Linear(dim_V, dim_V)
        self.gate = None
        if gated:
            self.gate = nn.Sequential(nn.Linear(dim_Q, dim_V), nn.SiLU())


class _IlraGAB(nn.Module):
    def __init__(self, dim_in, dim_out, num_heads, num_inds, ln=False):
        super().__init__()
        self.latent = nn.Parameter(torch.Tensor(1, num_inds, dim_out))
        nn.init.xavier_uniform_(self.latent)
        self.project_forward = _IlraMHA(dim_out, dim_in, dim_out, num_heads, ln=ln, gated=True)
        self.project_backward = _IlraMHA(dim_in, dim_out, dim_out, num_heads, ln=ln, gated=True)


class _IlraNLP(nn.Module):
    def __init__(self, dim, num_heads, num_seeds, ln=False):
        super().__init__()
        self.S = nn.Parameter(torch.Tensor(1, num_seeds, dim))
        nn.init.xavier_uniform_(self.S)
        self.mha = _IlraMHA(dim, dim, dim, num_heads, ln=ln)


def _d(t):
    return t.double()


class ILRA(nn.Module):
    """ILRA with the reference's constructor, initialisation and state-dict keys (``gab_blocks.{i}.latent``,
    ``gab_blocks.{i}.project_{forward,backward}.*``, ``pooling.S``, ``pooling.mha.*``, ``classifier.*``); the modules hold parameters
    only.  For ``topk = 1`` the model is, per block, ONE softmax pooling of the rows against eight effective queries (one latent, eight
    heads: ``E_h = (Wik_h Wk)^T q'_h / sqrt(32)`` -- parameters only, computed once per call), a [1, 256]-sized tail, and one row map
    (``project_backward`` has a single key, so every row gets the same attention output c: ``u = Wq x + bq + c``, ``xhat = (u +
    relu(Wo u + bo)) * silu(Wg x + bg)``); then the same pooling over the last block's rows and the classifier.  The two N-sized
    operations are HIP (csrc/ilra.hip), forward and backward; the tails are torch ops on [B, 8, d] / [B, 256] tensors EVALUATED IN
    FLOAT64 (fp32 parameters cast in the graph, autocast switched off), so every parameter gets its gradient through ordinary autograd.
    ``fc_k`` and the q / k thirds of ``in_proj`` of ``project_backward`` get exact zeros, as the reference's autograd gives.

    Served: ``dim_in = 512``, ``dim_hid = 256``, ``num_heads = 8``, ``topk = 1``, ``ln = False``, ``num_layers >= 1``, any ``num_cls``;
    anything else constructs (checkpoints load) and raises ``VlsaNativeError`` from ``forward``.  Bags are bf16 or fp32 device rows without
    a gradient of their own.  There is no dropout: ``train()`` and ``eval()`` compute the same."""

    ROW_BUDGET = 1 << 20          # rows per chunk of forward_bags (a bigger bag travels alone): bounds the packed activations

    def __init__(self, dim_in=512, dim_hid=256, num_cls=2, num_layers=2, num_heads=8, topk=1, ln=False, **kwargs):
        super().__init__()
        self.cfg = dict(dim_in=dim_in, dim_hid=dim_hid, num_layers=num_layers, num_heads=num_heads, topk=topk, ln=ln)
        self.gab_blocks = nn.ModuleList([_IlraGAB(dim_in=dim_in if i == 0 else dim_hid, dim_out=dim_hid, num_heads=num_heads, num_inds=topk,
                                                  ln=ln) for i in range(num_layers)])
        self.pooling = _IlraNLP(dim=dim_hid, num_heads=num_heads, num_seeds=topk, ln=ln)
        self.classifier = nn.Linear(in_features=dim_hid, out_features=num_cls)
        _ilra_initialize_weights(self)
        print("[setup] initialized an ILRA model.")

    def _check_served(self):
        c = self.cfg
        if (c["dim_in"], c["dim_hid"], c["num_heads"], c["topk"], bool(c["ln"])) != (512, 256, 8, 1, False) or c["num_layers"] < 1:
            raise VF.VlsaNativeError(f"ILRA: the HIP kernels cover dim_in = 512, dim_hid = 256, num_heads = 8, topk = 1, ln = False, "
                                     f"num_layers >= 1 (got {c}); there is no other route")

    @staticmethod
    def _queries(mha, seed):
        """(fc_q(seed) [256], E [8, d]) of an attention block whose query is the one row ``seed`` [1, 1, 256], in float64"""
        a = mha.multihead_attn
        Wi, bi = _d(a.in_proj_weight), _d(a.in_proj_bias)
        qf = F.linear(_d(seed).view(1, 256), _d(mha.fc_q.weight), _d(mha.fc_q.bias))[0]              # the "Q" of O = Q + A
        qf = qf + 0.0 * _d(mha.fc_k.bias).sum()          # the key biases are constant over the rows and cancel in the softmax: exact zeros
        qp = F.linear(qf, Wi[:256], bi[:256])
        M = Wi[256:512] @ _d(mha.fc_k.weight)                                                           # [256, d]
        E = (qp.view(8, 32, 1) * M.view(8, 32, -1)).sum(1) / math.sqrt(32.0)
        return qf, E

    @staticmethod
    def _tail(mha, qf, Z, seed):
        """[B, 256] behind the pooling Z [B, 8, d] (float64): values, per-head pick, out_proj, residual, fc_o, gate"""
        a = mha.multihead_attn
        Wi, bi = _d(a.in_proj_weight), _d(a.in_proj_bias)
        v = F.linear(F.linear(Z, _d(mha.fc_v.weight), _d(mha.fc_v.bias)), Wi[512:], bi[512:])           # [B, 8, 256]
        B = v.shape[0]
        A = v.view(B, 8, 8, 32).diagonal(dim1=1, dim2=2).permute(0, 2, 1).reshape(B, 256)             # head h's 32 entries of row h
        O = qf[None, :] + F.linear(A, _d(a.out_proj.weight), _d(a.out_proj.bias))
        O = O + torch.relu(F.linear(O, _d(mha.fc_o.weight), _d(mha.fc_o.bias)))
        if mha.gate is not None:
            g = mha.gate._modules["0"]
            O = O * F.silu(F.linear(_d(seed).view(1, 256), _d(g.weight), _d(g.bias)))
        return O

    def _chunk(self, bags, prep, ret_state):
        """logits [B, num_cls] of one chunk of <= 64 bags; prep: the per-call (qf, E) of every block and of the pooling"""
        xp, state = None, {}
        for i, blk in enumerate(self.gab_blocks):
            pf, pb = blk.project_forward, blk.project_backward
            qf, E = prep[i]
            Z = VF.ilra_pool_bags(bags, E.float(), xp)
            H = self._tail(pf, qf, Z.double(), blk.latent)
            a = pb.multihead_attn
            c = F.linear(F.linear(F.linear(H, _d(pb.fc_v.weight), _d(pb.fc_v.bias)), _d(a.in_proj_weight)[512:], _d(a.in_proj_bias)[512:]),
                         _d(a.out_proj.weight), _d(a.out_proj.bias))
            # fc_k of project_backward feeds a softmax over ONE key: it joins the graph with weight 0, so that it receives the exact zeros
            # the reference's autograd gives (an optimizer with weight decay treats a missing gradient and a zero one differently)
            c = c + 0.0 * (_d(pb.fc_k.weight).sum() + _d(pb.fc_k.bias).sum())
            btil = (_d(pb.fc_q.bias)[None, :] + c).float()
            g = pb.gate._modules["0"]
            out = VF.ilra_rowmap_bags(bags, pb.fc_q.weight, btil, pb.fc_o.weight, pb.fc_o.bias, g.weight, g.bias, xp, ret_mask=ret_state)
            xp, mask = out if ret_state else (out, None)
            if ret_state:
                state[f"Z{i}"], state[f"H{i}"], state[f"mask{i}"], state[f"xhat{i}"] = Z, H, mask, xp
        qf, E = prep[-1]
        Z = VF.ilra_pool_bags(bags, E.float(), xp)
        feat = self._tail(self.pooling.mha, qf, Z.double(), self.pooling.S)
        logits = F.linear(feat, _d(self.classifier.weight), _d(self.classifier.bias)).float()
        if ret_state:
            state["Zp"], state["feat"] = Z, feat
        return logits, state

    def forward_bags(self, bags, ret_state=False):
        """logits [B, num_cls] of a list of bags ([N_i, 512] or [1, N_i, 512], bf16 or fp32 device rows) or a ``BagSet``:
        ``torch.cat([self(x) for x in bags])``, in chunks of <= 64 bags and <= ROW_BUDGET rows per launch chain.  A ``BagSet`` is taken
        as it is (no per-bag checks, no host synchronisation, no staging upload once its descriptor table is up).  ret_state: also a
        list of per-chunk dicts (Z{i}, H{i}, mask{i}, xhat{i} per block, Zp, feat)."""
        self._check_served()
        if len(bags) == 0:
            raise ValueError("forward_bags needs at least one bag")
        if not isinstance(bags, VF.BagSet):
            bags = VF.checked_bags(bags, 512, "ILRA takes non-empty bags with 512 features, one dtype (bf16 or fp32) and one device",
                                   non_empty=True, no_grad="ILRA: the bag requires grad, but bag rows receive no gradient from the HIP kernels")
        VF._need_gpu(self.classifier.weight)
        with torch.autocast(device_type="cuda", enabled=False):
            prep = [self._queries(blk.project_forward, blk.latent) for blk in self.gab_blocks]
            prep.append(self._queries(self.pooling.mha, self.pooling.S))
            outs, states = zip(*[self._chunk(chunk, prep, ret_state) for chunk in VF.bag_chunks(bags, 64, self.ROW_BUDGET)])
        logits = VF.cat(outs)
        return (logits, list(states)) if ret_state else logits

    def forward(self, X):
        return self.forward_bags([X])

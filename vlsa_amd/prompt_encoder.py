"""Text tower of the VL model on the GPU: drop-in counterpart of the reference's ``CONCHPromptEncoder``
(model/prompt_encoder.py:209-322) -- same constructor contract (wraps a CoCa model's ``.text`` tower), same attribute
and state-dict names (``positional_embedding``, ``cls_emb``, ``transformer.resblocks.N.{ln_1,attn,ln_2,mlp}.*``,
``ln_final.*``, ``text_projection``, ``token_embedding.weight``), same ``forward(prompts_text | prompts_embedding,
prompts_pseudo_tokens)`` -> ``[n_prompts, output_dim]``.

The 12 pre-LN blocks run in libvlsa_hip.so (vlsa_amd/csrc/text_tower.hip) on the COMPACT rows of the prompts: only the
positions that can reach the pooled CLS token are evaluated (a 13-row problem per rank prompt instead of 128 -- exact, see
the kernel file), f32 MFMA throughout.  Differentiable w.r.t. ``prompts_embedding`` (the learnable context / rank
embeddings of the prompt learner); the tower itself is frozen in every shipped configuration
(``vlsa_txt_encoder_frozen: True``, cfg_vlsa_conch.yaml:69).  A tower whose own parameters require grad
(``vlsa_txt_encoder_frozen: False``) runs the same kernels plus the weight-gradient products of ``vlsa_tt_backward_train``
(``_TextTowerTrainFn``; until round 4 that case was a torch route).

``CLIPPromptEncoder`` and ``HFCLIPPromptEncoder`` (model/prompt_encoder.py:35-207) are the same machinery (``HipTextTower``: row plans,
packed weights, the two autograd functions) over the CLIP text tower -- OpenAI's layout and HuggingFace's: QuickGELU in the MLP, no
CLS token, the ``<eot>`` row pooled (``vlsa_tt_model.flags``, include/vlsa_hip.h).  Their compact rows are positions 0 .. <eot>.
"""
from __future__ import annotations

import ctypes
import functools
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _native as nat
from ._native import VlsaNativeError


_TTLayer, _TTModel, _TTRows = (nat.STRUCTS[n] for n in ("vlsa_tt_layer", "vlsa_tt_model", "vlsa_tt_rows"))     # include/vlsa_hip.h


# -- parameter holders with the reference's names (model/conch/transformer.py:191-247,290-322) ---------------------------
class _SelfAttention(nn.Module):          # the parameters of nn.MultiheadAttention(width, heads)
    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)


class QuickGELU(nn.Module):               # model/clip/model.py:166-168 (a marker here: the kernels evaluate it)
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _Block(nn.Module):
    def __init__(self, width, act=nn.GELU):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = _SelfAttention(width)
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, 4 * width)), ("gelu", act()),
                                              ("c_proj", nn.Linear(4 * width, width))]))


class _Transformer(nn.Module):
    def __init__(self, width, layers, heads, act=nn.GELU):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.ModuleList([_Block(width, act) for _ in range(layers)])


def compact_rows(pseudo_tokens: torch.Tensor, ctx_len: int, prefix_len: int = 0):
    """Host-side row plan for a [n, ctx_len - 1] pseudo-token matrix (0 = pad).  The CLS row (appended last) may attend to
    column 0 and to column j + 1 for every non-pad token j (build_cls_mask, model/prompt_encoder.py:245-252: the pad mask is
    shifted right by one); token rows are causal.  Prompt s therefore needs positions 0..m_s (m_s = last column < ctx_len - 1
    the CLS row can see) plus the CLS row.

    prefix_len = L > 0: the caller guarantees that positions 0 .. L-1 carry the same embedding in every prompt (<sot> and the
    shared context tokens of the CoOp learners).  Under the causal mask those rows are identical in every layer, so they are
    planned ONCE (rows 0 .. L-1) and prompt s keeps only positions L .. m_s + its CLS row; every CLS row must see all L prefix
    positions (true for real tokens) and every prompt must reach past the prefix, else the plan falls back to L = 0.
    Returns dict of int lists (+ 'prefix_len': the L actually used)."""
    pt = pseudo_tokens.detach().to("cpu")
    n, L_tok = pt.shape
    if L_tok != ctx_len - 1:
        raise ValueError(f"expected {ctx_len - 1} token positions, got {L_tok}")
    keeps, ms = [], []
    for s in range(n):
        keep = [True] + [bool(v) for v in (pt[s] != 0).tolist()]          # keep[c]: CLS attends to column c (c = L_tok: itself)
        keeps.append(keep)
        ms.append(max(c for c in range(L_tok) if keep[c]))
    L = int(prefix_len or 0)
    if L > 0 and not (n > 1 and all(m >= L for m in ms) and all(all(k[:L]) for k in keeps)):
        L = 0
    row_seq, row_pos, row_src, seq_row0, cls_keep = [], [], [], [], []
    for c in range(L):                                                    # the shared prefix, once
        row_seq.append(0); row_pos.append(c); row_src.append(c); cls_keep.append(1)
    seq_row0.append(len(row_seq))
    max_len = 0
    for s in range(n):
        keep, m = keeps[s], ms[s]
        for c in range(L, m + 1):
            row_seq.append(s); row_pos.append(c); row_src.append(c); cls_keep.append(1 if keep[c] else 0)
        row_seq.append(s); row_pos.append(ctx_len - 1); row_src.append(-1); cls_keep.append(1 if keep[L_tok] else 0)
        seq_row0.append(len(row_seq))
        max_len = max(max_len, m + 2)                                     # keys of the prompt's CLS row incl. the prefix
    return dict(row_seq=row_seq, row_pos=row_pos, row_src=row_src, seq_row0=seq_row0, cls_keep=cls_keep, max_len=max_len,
                n_seq=n, M=len(row_seq), prefix_len=L)


def last_token_rows(pseudo_tokens: torch.Tensor, ctx_len: int, prefix_len: int = 0, refuse_gaps: bool = False):
    """Host-side row plan for a [n, L] pseudo-token matrix of a tower WITHOUT a CLS slot (the CLIP towers; L <= ctx_len: HuggingFace
    pads to the longest sentence and takes ``position_embedding[:L]``).  The pooled row of prompt s is position m_s = ``argmax`` of its
    row (the reference's pooling index, model/prompt_encoder.py:90,199-203: the <eot> token); under the causal mask it sees positions
    0 .. m_s and nothing behind it, so the prompt's rows are positions 0 .. m_s, the LAST one pooled (``VLSA_TT_POOL_LAST_TOKEN``).
    Every row is a token row (``row_src`` = its position), ``cls_keep`` is all ones (the attention kernels' "last row" is then causal
    like the others), ``max_len`` = m_s + 1 keys.  ``prefix_len`` as in ``compact_rows``: positions 0 .. L-1 once, if every prompt
    reaches past them (m_s >= L) and there is more than one prompt, else the plan falls back to L = 0.
    refuse_gaps: a zero in front of a row's maximum is an error (HuggingFace masks that KEY for every query; the plan cannot)."""
    pt = pseudo_tokens.detach().to("cpu")
    n, L_tok = pt.shape
    if not 2 <= L_tok <= ctx_len:
        raise ValueError(f"expected 2 .. {ctx_len} token positions, got {L_tok}")
    ms = [int(m) for m in pt.argmax(dim=-1).tolist()]
    if min(ms) < 1:
        raise ValueError("a prompt's pooled position is 0: a sentence holds at least <sot> and <eot>")
    if refuse_gaps:
        for s_, m in enumerate(ms):
            if bool((pt[s_, :m] == 0).any()):
                raise NotImplementedError(f"pseudo-tokens of prompt {s_} have a zero in front of their maximum (position {m}): the "
                                          "HuggingFace tower masks that key for every query, which the compact-row plan cannot express")
    L = int(prefix_len or 0)
    if L > 0 and not (n > 1 and all(m >= L for m in ms)):
        L = 0
    row_seq, row_pos = [0] * L, list(range(L))
    seq_row0 = [L]
    for s_, m in enumerate(ms):
        row_seq += [s_] * (m + 1 - L)
        row_pos += list(range(L, m + 1))
        seq_row0.append(len(row_seq))
    return dict(row_seq=row_seq, row_pos=row_pos, row_src=list(row_pos), seq_row0=seq_row0, cls_keep=[1] * len(row_seq),
                max_len=max(ms) + 1, n_seq=n, M=len(row_seq), prefix_len=L)


class _RowPlan:
    """Device copies of the compact-row tables + the C struct, cached per pseudo-token pattern."""

    def __init__(self, pseudo_tokens, ctx_len, device, prefix_len=0, planner=compact_rows):
        rp = planner(pseudo_tokens, ctx_len, prefix_len)
        self.n_seq, self.M, self.max_len, self.prefix_len = rp["n_seq"], rp["M"], rp["max_len"], rp["prefix_len"]
        self.M_pad = (self.M + 95) // 96 * 96      # whole 16-, 32- and 48-row workgroup tiles
        pad = self.M_pad - self.M
        i32 = lambda v, fill: torch.tensor(v + [fill] * pad, dtype=torch.int32).to(device)   # noqa: E731
        self.row_seq, self.row_pos, self.row_src = i32(rp["row_seq"], 0), i32(rp["row_pos"], 0), i32(rp["row_src"], -1)
        self.seq_row0 = torch.tensor(rp["seq_row0"], dtype=torch.int32).to(device)
        self.cls_keep = torch.tensor(rp["cls_keep"] + [0] * pad, dtype=torch.uint8).to(device)
        self.c = _TTRows(self.n_seq, self.M, self.M_pad, self.max_len, self.row_seq.data_ptr(), self.row_pos.data_ptr(),
                         self.row_src.data_ptr(), self.seq_row0.data_ptr(), self.cls_keep.data_ptr(), self.prefix_len)
        self.ws = None    # inference workspace (no activations kept), allocated on first use
        self._rp = rp
        self._status = []  # (pinned int32[4], event): status words of persistent launches on their way to the host
        self.ws_free = {}  # (bytes, stream) -> workspaces of finished forward + backward passes, ready for the next training forward

    def watch_status(self, words: torch.Tensor):
        host = torch.empty(4, dtype=torch.int32).pin_memory()
        host.copy_(words, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._status.append((host, ev))
        if len(self._status) > 64:
            self.check_status(wait=True)

    def check_status(self, wait: bool = False):
        """Raise if a persistent text-tower launch reported a timed-out in-kernel wait (vlsa_tt_status_offset): its text features
        -- and everything computed from them -- are void."""
        keep = []
        for host, ev in self._status:
            if wait:
                ev.synchronize()
            if not ev.query():
                keep.append((host, ev))
                continue
            code, stage, wg, seen = (int(v) for v in host)
            if code != 0:
                self._status = []
                raise VlsaNativeError(f"text tower: the persistent forward launch timed out in stage {stage} (workgroup {wg}, counter {seen}): "
                                      "not all of its workgroups were resident (another kernel held CUs).  Its outputs are void; "
                                      "VLSA_TT_PERSIST=0 selects the launch-per-stage path")
        self._status = keep


class _TextTowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, enc, plan):
        lib = nat.load()
        model = enc._c_model(emb.device)
        save = 1 if ctx.needs_input_grad[0] else 0
        nbytes = lib.vlsa_tt_workspace_bytes(ctypes.byref(model), ctypes.byref(plan.c), save)
        if nbytes == 0:
            raise VlsaNativeError("text tower: unsupported shape (width % 128, width <= 768, 64 features per head, <= 128 rows per prompt)")
        if save:
            # holds the activations until backward; taken from the plan's pool of workspaces a finished backward handed back (same
            # stream: ordered behind that backward's kernels) -- a fresh one costs a 41 MB fill per step (15 us, round 4)
            key = (nbytes, torch.cuda.current_stream(emb.device).cuda_stream)
            free = plan.ws_free.get(key)
            ws = free.pop() if free else torch.zeros(nbytes, dtype=torch.uint8, device=emb.device)
            ctx.ws_key = key
        else:
            if plan.ws is None or plan.ws.numel() < nbytes:
                plan.ws = torch.zeros(nbytes, dtype=torch.uint8, device=emb.device)
            ws = plan.ws
        x = emb.detach()
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        out = torch.empty(plan.n_seq, enc.output_dim, dtype=torch.float32, device=emb.device)
        s = ctypes.c_void_p(torch.cuda.current_stream(emb.device).cuda_stream)
        packed = enc._packed_weights(emb.device, with_backward=bool(save))
        plan.check_status()                  # a time-out of an EARLIER persistent launch (see below) surfaces here at the latest
        # opt-in persistent forward: asked for per call through a flag bit -- the switch lives HERE (VLSA_TT_PERSIST=1, read per call:
        # tests and benches flip it inside one process); libvlsa_hip.so reads no environment
        flags = save | (nat.TT_PERSISTENT if os.environ.get("VLSA_TT_PERSIST", "0") not in ("", "0") else 0)
        nat.check(lib.vlsa_tt_forward(ctypes.byref(model), ctypes.byref(plan.c), ctypes.c_void_p(packed.data_ptr()),
                                      ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), ctypes.c_void_p(ws.data_ptr()), flags,
                                      ctypes.c_void_p(out.data_ptr()), s), "vlsa_tt_forward")
        off = lib.vlsa_tt_status_offset(ctypes.byref(model), ctypes.byref(plan.c), flags)
        if off >= 0:
            # the persistent launch reports a timed-out wait in its workspace: read the four words back WITHOUT stalling the
            # caller (pinned buffer + event) and look at them once the copy has landed -- here at the next call, in backward,
            # or through ``check_status(wait=True)``
            plan.watch_status(ws[off:off + 16].view(torch.int32))
        if save:
            ctx.ws, ctx.plan, ctx.enc, ctx.shape, ctx.packed = ws, plan, enc, tuple(emb.shape), packed
        ctx.keep = x
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = nat.load()
        enc, plan = ctx.enc, ctx.plan
        plan.check_status()
        model = enc._c_model(dout.device)
        g = dout.detach().float().contiguous()
        demb = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        s = ctypes.c_void_p(torch.cuda.current_stream(dout.device).cuda_stream)
        nat.check(lib.vlsa_tt_backward(ctypes.byref(model), ctypes.byref(plan.c), ctypes.c_void_p(ctx.packed.data_ptr()),
                                       ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(ctx.ws.data_ptr()),
                                       ctypes.c_void_p(demb.data_ptr()), demb.stride(0), demb.stride(1), demb.numel(), s),
                  "vlsa_tt_backward")
        if torch.cuda.current_stream(dout.device).cuda_stream == ctx.ws_key[1]:
            free = plan.ws_free.setdefault(ctx.ws_key, [])
            if len(free) < 2:
                free.append(ctx.ws)          # (the kernels leave their tickets / counters zeroed: reusable as it is)
        ctx.ws = ctx.packed = None
        return demb, None, None


class _TextTowerTrainFn(torch.autograd.Function):
    """The tower with its OWN parameters under training (``vlsa_txt_encoder_frozen: False``, runner/vlsa_handler.py:131; off in
    every shipped configuration).  Same kernels as ``_TextTowerFn``; the forward keeps every block's attention output
    (``save_for_backward == 2``) and the backward is ONE C call (``vlsa_tt_backward_train``) that writes d prompts_embedding and
    the gradient of every tower parameter -- four dW = dY^T act products per block over the compact rows on the f32 matrix pipe,
    bias / LayerNorm gradients as fixed-order column sums (vlsa_amd/csrc/text_tower.hip: k_tt_dw).  ``tensors`` = the tower's
    parameters in ``_tower_tensors`` order (autograd inputs: their ``.grad`` is what the optimizer reads)."""

    @staticmethod
    def forward(ctx, emb, enc, plan, *tensors):
        lib = nat.load()
        model = enc._c_model(emb.device)
        nbytes = lib.vlsa_tt_workspace_bytes(ctypes.byref(model), ctypes.byref(plan.c), 2)
        if nbytes == 0:
            raise VlsaNativeError("text tower: unsupported shape (width % 128, width <= 768, 64 features per head, <= 128 rows per prompt)")
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=emb.device)
        x = emb.detach()
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        out = torch.empty(plan.n_seq, enc.output_dim, dtype=torch.float32, device=emb.device)
        s = ctypes.c_void_p(torch.cuda.current_stream(emb.device).cuda_stream)
        packed = enc._packed_weights(emb.device, with_backward=True)       # of the CURRENT weights (keyed on their versions)
        nat.check(lib.vlsa_tt_forward(ctypes.byref(model), ctypes.byref(plan.c), ctypes.c_void_p(packed.data_ptr()),
                                      ctypes.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), ctypes.c_void_p(ws.data_ptr()), 2,
                                      ctypes.c_void_p(out.data_ptr()), s), "vlsa_tt_forward")
        ctx.ws, ctx.plan, ctx.enc, ctx.shape, ctx.packed = ws, plan, enc, tuple(emb.shape), packed
        ctx.versions = [t._version for t in tensors]
        ctx.keep = x
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = nat.load()
        enc, plan = ctx.enc, ctx.plan
        slots = enc._tower_tensors()                        # (slot 1 is None for a tower without a CLS token)
        ts = [t for t in slots if t is not None]
        if [t._version for t in ts] != ctx.versions:
            raise RuntimeError("text tower: a weight was modified in place between forward and backward (the packed copies the "
                               "backward reads belong to the forward's weights)")
        model = enc._c_model(dout.device)
        g = dout.detach().float().contiguous()
        demb = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        # one allocation for all parameter gradients, handed out as views shaped like the parameters; the C struct mirrors _c_model
        sizes = [t.numel() for t in ts]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dout.device)
        grads, o = [], 0
        for t, n in zip(ts, sizes):
            grads.append(flat[o:o + n].view(t.shape))
            o += n
        it = iter(grads)
        ptr = [next(it).data_ptr() if t is not None else None for t in slots]      # gradient buffers in the C struct's slot order
        nl = (len(slots) - 5) // 12
        arr = (_TTLayer * nl)()
        for i in range(nl):
            for j, (name, _) in enumerate(_TTLayer._fields_):
                setattr(arr[i], name, ptr[5 + 12 * i + j])
        gm = _TTModel(model.width, model.heads, model.layers, model.out_dim, model.ctx_len, arr, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4],
                      model.flags)
        s = ctypes.c_void_p(torch.cuda.current_stream(dout.device).cuda_stream)
        nat.check(lib.vlsa_tt_backward_train(ctypes.byref(model), ctypes.byref(plan.c), ctypes.c_void_p(ctx.packed.data_ptr()),
                                             ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(ctx.ws.data_ptr()),
                                             ctypes.c_void_p(demb.data_ptr()), demb.stride(0), demb.stride(1), demb.numel(),
                                             ctypes.byref(gm), s), "vlsa_tt_backward_train")
        ctx.ws = ctx.packed = None
        need = ctx.needs_input_grad
        return (demb if need[0] else None, None, None) + tuple(gr if need[3 + i] else None for i, gr in enumerate(grads))


class HipTextTower(nat.TransientCaches, nn.Module):
    """What the three encoders share: the C-side view of a tower's weights (``_c_model``), their packed copies, the row plans and the
    route into ``_TextTowerFn`` / ``_TextTowerTrainFn``.  A subclass provides the reference's attributes plus ``heads``,
    ``context_length``, ``output_dim``, ``_tower_tensors()`` -- the parameters in the slot order of ``vlsa_tt_model`` (positional
    embedding, CLS embedding or None, ln_final weight / bias, text projection [width, out], then twelve per block in ``vlsa_tt_layer``
    order) -- and, for a tower without a CLS token, ``_tt_flags`` / ``_planner``."""

    _transient = {"_cm": lambda: None, "_cm_key": lambda: None, "_cm_arr": None, "_plans": dict, "_pk": lambda: None, "_pk_key": lambda: None,
                  "_pk_bwd": lambda: False, "_tt_cache": None, "_plan_last": None}
    _tt_flags = 0                                  # vlsa_tt_model.flags
    _planner = staticmethod(compact_rows)
    _plan_by_value = False                         # the plan depends on the pseudo-tokens' VALUES (argmax), not only on which are zero
    _activations = {"gelu": 0}                     # MLP activations the tower may have -> VLSA_TT_ACT_* bit
    _block_name = "the CONCH text block only (LayerNorm eps 1e-5, erf GELU, no LayerScale, mlp ratio 4, causal attention)"

    def _init_caches(self):
        self._cm, self._cm_key, self._plans = None, None, {}
        self._pk, self._pk_key, self._pk_bwd = None, None, False

    def _check_architecture(self, tower):
        """The kernels hard-code the CoCa text block of model/conch/transformer.py:191-247: pre-LN with eps 1e-5, exact (erf)
        GELU -- or, for the towers that list it in ``_activations``, QuickGELU -- no LayerScale, MLP ratio 4, causal mask.  Anything
        else would give wrong text features silently: refuse it.  Returns the activation's ``VLSA_TT_ACT_*`` bit."""
        def bad(what):
            raise NotImplementedError(f"text tower: {what} -- the HIP tower implements {self._block_name}")
        acts = set()
        width = self.positional_embedding.shape[1]
        lns = [self.ln_final]
        masks = [] if getattr(tower, "attn_mask", None) is None else [tower.attn_mask]
        for blk in self.transformer.resblocks:
            lns += [blk.ln_1, blk.ln_2]
            for name in ("ls_1", "ls_2"):
                ls = getattr(blk, name, None)
                if ls is not None and not isinstance(ls, nn.Identity):
                    bad(f"LayerScale ({name})")
            if getattr(blk, "ln_1_kv", None) is not None:
                bad("a cross-attention block")
            act = getattr(blk.mlp, "gelu", None)
            kind = ("gelu" if isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none"
                    else "quick_gelu" if type(act).__name__ == "QuickGELU" else None)
            if kind not in self._activations:
                bad(f"activation {type(act).__name__}")
            acts.add(kind)
            if getattr(blk, "attn_mask", None) is not None:
                masks.append(blk.attn_mask)
            if blk.mlp.c_fc.out_features != 4 * width or blk.mlp.c_proj.in_features != 4 * width:
                bad("mlp ratio != 4")
        for ln in lns:
            if abs(float(ln.eps) - 1e-5) > 1e-12 or not getattr(ln, "elementwise_affine", True):
                bad(f"LayerNorm eps {ln.eps}")
        for mask in masks:
            n = mask.shape[-1]
            causal = torch.full((n, n), float("-inf")).triu_(1)
            if not torch.equal(mask.detach().float().cpu(), causal):
                bad("a non-causal attention mask")
        if len(acts) > 1:
            bad("blocks with different activations")
        return self._activations[acts.pop()] if acts else 0

    # -- C-side view of the weights ------------------------------------------------------------------------------------
    def _tower_tensors(self):
        # cached: ~300 nn.Module attribute look-ups per call otherwise, several calls per step.  The Parameter objects survive
        # .to(device) / load_state_dict (in-place), whose effects the callers' (data_ptr, _version) keys still see; re-assigning a
        # parameter attribute is caught by the identity check on the first and last tensors.
        blocks = self.transformer.resblocks
        c = self.__dict__.get("_tt_cache")
        if (c is not None and c[0] == len(blocks) and c[1][0] is self.positional_embedding and c[1][4] is self.text_projection
                and (len(blocks) == 0 or c[1][-1] is blocks[len(blocks) - 1].mlp.c_proj.bias)):
            return c[1]
        ts = [self.positional_embedding, self.cls_emb, self.ln_final.weight, self.ln_final.bias, self.text_projection]
        for blk in blocks:
            ts += [blk.ln_1.weight, blk.ln_1.bias, blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight,
                   blk.attn.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias,
                   blk.mlp.c_proj.weight, blk.mlp.c_proj.bias]
        self.__dict__["_tt_cache"] = (len(blocks), ts)
        return ts

    def _c_model(self, device):
        ts = self._tower_tensors()
        ptr = [None if t is None else t.data_ptr() for t in ts]
        key = (tuple(ptr), self._tt_flags)
        if self._cm is not None and key == self._cm_key:
            return self._cm
        for t in ts:
            if t is None:
                continue
            if not t.is_cuda or t.device != device:
                raise VlsaNativeError("the text tower runs on the MI355X only: its weights must be on the device of the prompts "
                                      "(there is no CPU fallback)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise VlsaNativeError("text tower weights must be contiguous fp32 tensors")
        blocks = range((len(ts) - 5) // 12)
        arr = (_TTLayer * len(blocks))()
        for i in blocks:
            for j, name in enumerate(n for n, _ in _TTLayer._fields_):
                setattr(arr[i], name, ptr[5 + 12 * i + j])
        self._cm = _TTModel(ts[0].shape[1], self.heads, len(blocks), self.output_dim, self.context_length, arr, ptr[0], ptr[1], ptr[2],
                            ptr[3], ptr[4], self._tt_flags)
        self._cm_arr, self._cm_key = arr, key
        return self._cm

    def _packed_weights(self, device, with_backward: bool) -> torch.Tensor:
        """The tiled (MFMA-fragment-major) copies of the tower's matrices the product kernels read, rebuilt when a weight's
        storage or in-place version changes (load_state_dict, .to(device)); the backward set (transposes) only once a
        gradient is asked for."""
        ts = self._tower_tensors()
        mats = [ts[4]] + [ts[5 + 12 * i + j] for i in range((len(ts) - 5) // 12) for j in (2, 4, 8, 10)]   # projection, in / out / fc / proj
        key = tuple((t.data_ptr(), t._version) for t in mats)
        if self._pk is not None and self._pk_key == key and (self._pk_bwd or not with_backward):
            return self._pk
        lib = nat.load()
        model = self._c_model(device)
        nbytes = lib.vlsa_tt_packed_bytes(ctypes.byref(model), int(with_backward))
        if nbytes == 0:
            raise VlsaNativeError("text tower: unsupported shape (width % 128, width <= 768, 64 features per head, out_dim % 64)")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        nat.check(lib.vlsa_tt_pack_weights(ctypes.byref(model), ctypes.c_void_p(buf.data_ptr()), int(with_backward),
                                           ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "vlsa_tt_pack_weights")
        self._pk, self._pk_key, self._pk_bwd = buf, key, bool(with_backward)
        return buf

    def _plan(self, pseudo_tokens, device, prefix_len=0) -> _RowPlan:
        # fast path: the very tensor object (a learner's `pseudo_sentence_tokens` buffer) seen last time, unchanged in place;
        # otherwise keyed on CONTENT (the pattern of non-pad positions): `generate_pseudo_tokens` makes a new tensor per call
        prefix_len = int(prefix_len or 0)
        last = self.__dict__.get("_plan_last")
        if (last is not None and last[0] is pseudo_tokens and last[1] == pseudo_tokens._version and last[2].row_seq.device == device
                and last[3] == prefix_len):
            return last[2]
        content = pseudo_tokens.to("cpu", torch.int64) if self._plan_by_value else (pseudo_tokens != 0).to("cpu", torch.uint8)
        key = (bytes(content.contiguous().numpy().data), tuple(pseudo_tokens.shape), str(device), prefix_len)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) > 16:
                self._plans.clear()
            plan = _RowPlan(pseudo_tokens, self.context_length, device, prefix_len, self._planner)
            self._plans[key] = plan
        self.__dict__["_plan_last"] = (pseudo_tokens, pseudo_tokens._version, plan, prefix_len)
        return plan

    def _run(self, x, pseudo_tokens, prefix_len=0):
        """embeddings [n, L, width] on the device + their pseudo-tokens -> text features [n, output_dim] through the HIP tower"""
        if not x.is_cuda:
            raise VlsaNativeError("vlsa_amd runs on MI355X only: got CPU prompt embeddings (there is no CPU fallback; the CPU "
                                  "oracle under oracle/ is test infrastructure)")
        if x.dim() != 3 or pseudo_tokens.shape[0] != x.shape[0] or pseudo_tokens.shape[1] > x.shape[1]:
            raise ValueError(f"prompts_embedding {tuple(x.shape)} and prompts_pseudo_tokens {tuple(pseudo_tokens.shape)} do not belong "
                             "together (the row plan indexes the embeddings by the pseudo-tokens' positions)")
        plan = self._plan(pseudo_tokens, x.device, prefix_len)
        ts = [t for t in self._tower_tensors() if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
            return _TextTowerTrainFn.apply(x, self, plan, *ts)      # vlsa_txt_encoder_frozen: False
        return _TextTowerFn.apply(x, self, plan)


class CONCHPromptEncoder(HipTextTower):
    """``CONCHPromptEncoder(coca_model)`` adopts the text tower of a CoCa model exactly like the reference does
    (``coca_model.text.{positional_embedding, transformer, ln_final, cls_emb, text_projection, token_embedding, heads,
    pad_id}``, model/prompt_encoder.py:213-243); ``CONCHPromptEncoder(width=..., heads=..., layers=...)`` builds an empty tower
    of the CONCH text architecture to ``load_state_dict`` into (model/conch/model_configs/conch_ViT-B-16.json: 768 / 12 / 12,
    128 positions, 32007 tokens, 512 outputs)."""

    def __init__(self, coca_model=None, *, width: int = 768, heads: int = 12, layers: int = 12, context_length: int = 128,
                 vocab_size: int = 32007, output_dim: int = 512):
        super().__init__()
        if coca_model is not None:
            t = coca_model.text
            self.pad_id = t.pad_id
            assert self.pad_id == 0, "Assume pad_id = 0 in CONCH to encode prompts as expected."
            self.heads = t.heads
            self.positional_embedding = t.positional_embedding
            self.transformer = t.transformer
            self.ln_final = t.ln_final
            self.cls_emb = t.cls_emb
            self.text_projection = t.text_projection
            self.token_embedding = t.token_embedding
            if self.cls_emb is None:
                raise NotImplementedError("the CONCH text tower embeds a CLS token (embed_cls=True); towers without one are not supported")
            self._check_architecture(t)
        else:
            self.pad_id, self.heads = 0, heads
            self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
            self.transformer = _Transformer(width, layers, heads)
            self.ln_final = nn.LayerNorm(width)
            self.cls_emb = nn.Parameter(torch.empty(width))
            self.text_projection = nn.Parameter(torch.empty(width, output_dim))
            self.token_embedding = nn.Embedding(vocab_size, width)
            self.reset_parameters()
        self.context_length = self.positional_embedding.shape[0]
        self.output_dim = self.text_projection.shape[1]
        self.text_config = {"max_num_tokens": self.context_length - 1, "embedding_dim": self.token_embedding.embedding_dim,
                            "embedding_dtype": self.token_embedding.weight.dtype}
        self._init_caches()

    def reset_parameters(self):
        """TextTransformer.init_parameters (model/conch/transformer.py:376-392)."""
        d, L = self.transformer.width, self.transformer.layers
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        nn.init.normal_(self.cls_emb, std=0.01)
        proj_std, attn_std, fc_std = (d ** -0.5) * ((2 * L) ** -0.5), d ** -0.5, (2 * d) ** -0.5
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=d ** -0.5)

    # -- reference API ---------------------------------------------------------------------------------------------------
    def generate_pseudo_tokens(self, text):
        """1, 2, ... up to the token before the first pad, zeros behind it (model/prompt_encoder.py:257-265).  A row without
        any pad yields all zeros there (argmax of an all-False row is 0) -- kept as is."""
        first_pad = (text == self.pad_id).int().argmax(dim=-1)
        pos = torch.arange(text.shape[1], device=text.device)[None, :]
        return torch.where(pos < first_pad[:, None], pos + 1, torch.zeros_like(pos)).to(text.dtype)

    def forward(self, prompts_text=None, prompts_embedding=None, prompts_pseudo_tokens=None, shared_prefix_len=0):
        """prompts_text [n, 128] token ids (last slot = CLS placeholder) or prompts_embedding [n, 127, width] with
        prompts_pseudo_tokens [n, 127] (0 = pad) -> [n, output_dim]   (model/prompt_encoder.py:267-322).
        shared_prefix_len (beyond the reference's signature; 0 = off): the caller's promise that positions 0 .. L-1 hold the SAME
        embedding in every prompt (what the CoOp learners produce: <sot> + shared context, ``learner.shared_prefix_len``); those
        rows are then evaluated once for all prompts -- exact under the causal mask (see ``compact_rows``)."""
        L = self.context_length - 1
        if prompts_text is not None:
            assert prompts_text.shape[1] == L + 1, "Found invalid input of `prompts_text`."
            ids = prompts_text[:, :-1]                              # make space for the CLS token
            if prompts_pseudo_tokens is None:
                prompts_pseudo_tokens = self.generate_pseudo_tokens(ids)
            x = self.token_embedding(ids.to(self.token_embedding.weight.device))
        else:
            assert prompts_embedding is not None, "Found null `prompts_text`, please specify `prompts_embedding`."
            assert prompts_pseudo_tokens is not None, "Found null `prompts_text`, please specify `prompts_pseudo_tokens`."
            x = prompts_embedding
        assert x.shape[1] == L
        return self._run(x, prompts_pseudo_tokens, shared_prefix_len if prompts_text is None else 0)


def _eot_pseudo_tokens(text, idx_eot):
    """1 .. idx_eot + 1 on positions 0 .. idx_eot of every row, zeros behind (model/prompt_encoder.py:54-62,134-142)"""
    pos = torch.arange(text.shape[1], device=text.device)[None, :]
    return torch.where(pos <= idx_eot[:, None], pos + 1, torch.zeros_like(pos)).to(text.dtype)


class CLIPPromptEncoder(HipTextTower):
    """``CLIPPromptEncoder(clip_model)`` adopts the text side of an OpenAI CLIP model exactly like the reference does
    (``clip_model.{transformer, positional_embedding, ln_final, text_projection, token_embedding}``, model/prompt_encoder.py:35-52);
    ``CLIPPromptEncoder(width=..., heads=..., layers=...)`` builds an empty tower of the ViT-B text architecture to
    ``load_state_dict`` into (512 / 8 / 12, 77 positions, 49408 tokens, 512 outputs).

    The CLIP block is the CoCa block with QuickGELU in the MLP and without a CLS token: the pooled row is the ``<eot>`` row
    (``argmax`` of the pseudo-tokens), then ``ln_final`` and ``text_projection``.  The reference's loader hands fp16 weights
    (``convert_weights``, model/clip/model.py:375-396); the HIP tower computes in fp32, so adopted parameters are WIDENED to fp32
    in place at adoption -- exact, every fp16 value is an fp32 value -- and ``text_config['embedding_dtype']`` says fp32."""

    _tt_flags = nat.TT_ACT_QUICK_GELU | nat.TT_POOL_LAST_TOKEN
    _planner = staticmethod(last_token_rows)
    _plan_by_value = True
    _activations = {"quick_gelu": nat.TT_ACT_QUICK_GELU, "gelu": 0}
    _block_name = ("the CLIP text block only (LayerNorm eps 1e-5, QuickGELU or erf GELU, no LayerScale, mlp ratio 4, causal "
                   "attention)")
    cls_emb = None                                  # no CLS token: slot 1 of the C struct stays NULL

    def __init__(self, clip_model=None, *, width: int = 512, heads: int = 8, layers: int = 12, context_length: int = 77,
                 vocab_size: int = 49408, output_dim: int = 512):
        super().__init__()
        if clip_model is not None:
            self.transformer = clip_model.transformer
            self.positional_embedding = clip_model.positional_embedding
            self.ln_final = clip_model.ln_final
            self.text_projection = clip_model.text_projection
            self.token_embedding = clip_model.token_embedding
            for p in self.parameters():
                if p.dtype != torch.float32:
                    p.data = p.data.float()
            attn = self.transformer.resblocks[0].attn
            self.heads = int(getattr(attn, "num_heads", None) or getattr(self.transformer, "heads"))
            self._tt_flags = nat.TT_POOL_LAST_TOKEN | self._check_architecture(clip_model)
        else:
            self.heads = heads
            self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
            self.transformer = _Transformer(width, layers, heads, act=QuickGELU)
            self.ln_final = nn.LayerNorm(width)
            self.text_projection = nn.Parameter(torch.empty(width, output_dim))
            self.token_embedding = nn.Embedding(vocab_size, width)
            self.reset_parameters()
        self.context_length = self.positional_embedding.shape[0]
        self.output_dim = self.text_projection.shape[1]
        self.text_config = {"max_num_tokens": 77, "embedding_dim": self.token_embedding.embedding_dim,
                            "embedding_dtype": self.token_embedding.weight.dtype}
        self._init_caches()

    def reset_parameters(self):
        """CLIP.initialize_parameters (model/clip/model.py:299-326), text side."""
        d, L = self.transformer.width, self.transformer.layers
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std, attn_std, fc_std = (d ** -0.5) * ((2 * L) ** -0.5), d ** -0.5, (2 * d) ** -0.5
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=d ** -0.5)

    @property
    def dtype(self):
        return self.transformer.resblocks[0].mlp.c_fc.weight.dtype

    def generate_pseudo_tokens(self, text):
        """the <eot> token is the highest id of a sentence tokenised by OpenAI CLIP (model/prompt_encoder.py:54-62)"""
        return _eot_pseudo_tokens(text, text.argmax(dim=-1))

    def forward(self, prompts_text=None, prompts_embedding=None, prompts_pseudo_tokens=None, shared_prefix_len=0):
        """prompts_text [n, 77] token ids, or prompts_embedding [n, 77, width] with prompts_pseudo_tokens [n, 77] (their ``argmax`` is
        the pooled position) -> [n, output_dim]   (model/prompt_encoder.py:64-92).  ``shared_prefix_len`` as on the CONCH encoder."""
        L = self.text_config["max_num_tokens"]
        if prompts_text is not None:
            assert prompts_text.shape[1] == L, "Found invalid input of `prompts_text`."
            if prompts_pseudo_tokens is None:
                prompts_pseudo_tokens = self.generate_pseudo_tokens(prompts_text)
            x = self.token_embedding(prompts_text.to(self.token_embedding.weight.device))
        else:
            assert prompts_embedding is not None, "Found null `prompts_text`, please specify `prompts_embedding`."
            assert prompts_pseudo_tokens is not None, "Found null `prompts_text`, please specify `prompts_pseudo_tokens`."
            x = prompts_embedding
        assert x.shape[1] == self.context_length          # (the reference adds the whole positional_embedding)
        return self._run(x, prompts_pseudo_tokens, shared_prefix_len if prompts_text is None else 0)


class HFCLIPPromptEncoder(HipTextTower):
    """``HFCLIPPromptEncoder(hf_clip_model)`` adopts the text side of a ``transformers`` ``CLIPModel`` like the reference does
    (model/prompt_encoder.py:99-132) and keeps its parameters under HuggingFace's names: ``embeddings.*``,
    ``encoder.layers.N.{self_attn.{q,k,v,out}_proj, layer_norm1, layer_norm2, mlp.fc1, mlp.fc2}.*``, ``final_layer_norm.*``,
    ``text_projection.weight`` ([out, width]).  The kernels read a concatenated [3 width, width] in-projection (and its bias) per block
    and the projection's transpose: copies made here, rebuilt IN PLACE whenever a q / k / v / projection tensor's storage or version
    changes (the packed weights key on their version).

    ``hidden_act`` "quick_gelu" (openai/clip-*, vinid/plip) or "gelu" selects the kernels' activation; anything else the kernels do not
    compute -- another activation, a LayerNorm eps other than 1e-5, pseudo-tokens with a zero in front of their maximum (HuggingFace would
    mask that key) -- is refused with the reason.  The tower is FROZEN here: gradients flow to ``prompts_embedding``; a tower parameter
    that requires grad under grad mode raises ``NotImplementedError`` (its gradient would have to be split back into HuggingFace's
    q / k / v tensors; nothing is silently frozen)."""

    _planner = staticmethod(functools.partial(last_token_rows, refuse_gaps=True))
    _plan_by_value = True
    _transient = dict(HipTextTower._transient, _hf_cache=None, _hf_src=None)

    def __init__(self, hf_clip_model):
        super().__init__()
        text_model = hf_clip_model.text_model
        self.hf_text_config = cfg = text_model.config
        self.embeddings = text_model.embeddings
        self.encoder = text_model.encoder
        self.final_layer_norm = text_model.final_layer_norm
        self.eos_token_id = cfg.eos_token_id
        self.text_projection = hf_clip_model.text_projection
        self.token_embedding = text_model.embeddings.token_embedding

        def bad(what):
            raise NotImplementedError(f"text tower: {what} -- the HIP tower implements the CLIP text block only (LayerNorm eps 1e-5, "
                                      "quick_gelu or gelu, mlp ratio 4, causal attention, biased projections)")
        act = {"quick_gelu": nat.TT_ACT_QUICK_GELU, "gelu": 0}.get(cfg.hidden_act)
        if act is None:
            bad(f"hidden_act {cfg.hidden_act!r}")
        width = cfg.hidden_size
        lns = [self.final_layer_norm]
        for blk in self.encoder.layers:
            lns += [blk.layer_norm1, blk.layer_norm2]
            if blk.mlp.fc1.out_features != 4 * width:
                bad("mlp ratio != 4")
            for lin in (blk.self_attn.q_proj, blk.self_attn.k_proj, blk.self_attn.v_proj, blk.self_attn.out_proj, blk.mlp.fc1, blk.mlp.fc2):
                if lin.bias is None:
                    bad("a projection without bias")
        for ln in lns:
            if abs(float(ln.eps) - 1e-5) > 1e-12 or not getattr(ln, "elementwise_affine", True):
                bad(f"LayerNorm eps {ln.eps}")
        if float(getattr(cfg, "attention_dropout", 0.0) or 0.0) != 0.0:
            bad("attention dropout")
        if self.text_projection.bias is not None:
            bad("a text projection with bias")
        self._tt_flags = nat.TT_POOL_LAST_TOKEN | act
        self.heads = cfg.num_attention_heads
        self.context_length = self.embeddings.position_embedding.weight.shape[0]
        self.output_dim = self.text_projection.weight.shape[0]
        self.text_config = {"max_num_tokens": 77, "embedding_dim": self.token_embedding.embedding_dim,
                            "embedding_dtype": self.token_embedding.weight.dtype}
        self._init_caches()

    def _hf_sources(self):
        """HuggingFace's own tensors: [position embedding, final_layer_norm w / b, text_projection.weight], then 16 per block"""
        layers = self.encoder.layers
        c = self.__dict__.get("_hf_src")      # (cached like the base class's list: ~400 module attribute look-ups per call otherwise)
        if (c is not None and len(c) == 4 + 16 * len(layers) and c[0] is self.embeddings.position_embedding.weight
                and c[3] is self.text_projection.weight and (len(layers) == 0 or c[-1] is layers[len(layers) - 1].mlp.fc2.bias)):
            return c
        src = [self.embeddings.position_embedding.weight, self.final_layer_norm.weight, self.final_layer_norm.bias, self.text_projection.weight]
        for blk in layers:
            a = blk.self_attn
            src += [blk.layer_norm1.weight, blk.layer_norm1.bias, a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.q_proj.bias,
                    a.k_proj.bias, a.v_proj.bias, a.out_proj.weight, a.out_proj.bias, blk.layer_norm2.weight, blk.layer_norm2.bias,
                    blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias]
        self.__dict__["_hf_src"] = src
        return src

    def _tower_tensors(self):
        src = self._hf_sources()
        key = tuple((t.data_ptr(), t._version) for t in src)
        c = self.__dict__.get("_hf_cache")
        if c is not None and c[0] == key:
            return c[1]
        fresh = c is None or c[2] != tuple((t.device, t.dtype) for t in src)
        with torch.no_grad():
            # the derived operands: text_projection^T [width, out] and per block q | k | v stacked as nn.MultiheadAttention stores them;
            # written into the buffers of the last build when there is one (same storage, version bumped: what `_packed_weights` keys on)
            proj = src[3].t().contiguous() if fresh else c[1][4].copy_(src[3].t())
            ts = [src[0], None, src[1], src[2], proj]
            for i in range((len(src) - 4) // 16):
                b = src[4 + 16 * i:20 + 16 * i]
                if fresh:
                    in_w, in_b = torch.cat(b[2:5]), torch.cat(b[5:8])
                else:
                    in_w, in_b = c[1][5 + 12 * i + 2], c[1][5 + 12 * i + 3]
                    torch.cat(b[2:5], out=in_w)
                    torch.cat(b[5:8], out=in_b)
                ts += [b[0], b[1], in_w, in_b] + b[8:]
        self.__dict__["_hf_cache"] = (key, ts, tuple((t.device, t.dtype) for t in src))
        return ts

    def generate_pseudo_tokens(self, text):
        """the first ``eos_token_id`` of every row ends its sentence (model/prompt_encoder.py:134-142)"""
        return _eot_pseudo_tokens(text, (text.to(dtype=torch.int) == self.eos_token_id).int().argmax(dim=-1))

    def forward(self, prompts_text=None, prompts_embedding=None, prompts_pseudo_tokens=None, shared_prefix_len=0):
        """prompts_text [n, L] token ids, or prompts_embedding [n, L, width] with prompts_pseudo_tokens [n, L]; L <= 77 (HuggingFace's
        tokenizer pads to the longest sentence) -> [n, output_dim]   (model/prompt_encoder.py:144-207).  ``shared_prefix_len`` as on
        the CONCH encoder."""
        if torch.is_grad_enabled() and any(t.requires_grad for t in self._hf_sources()):
            raise NotImplementedError("HFCLIPPromptEncoder: a tower parameter requires grad -- the HuggingFace-layout tower runs frozen "
                                      "only (gradients go to `prompts_embedding`); freeze it (vlsa_txt_encoder_frozen: True) or use the "
                                      "OpenAI layout (CLIPPromptEncoder), whose tower trains")
        if prompts_text is not None:
            if prompts_pseudo_tokens is None:
                prompts_pseudo_tokens = self.generate_pseudo_tokens(prompts_text)
            x = self.token_embedding(prompts_text.to(self.token_embedding.weight.device))
        else:
            assert prompts_embedding is not None, "Found null `prompts_text`, please specify `prompts_embedding`."
            assert prompts_pseudo_tokens is not None, "Found null `prompts_text`, please specify `prompts_pseudo_tokens`."
            x = prompts_embedding
        assert x.shape[1] <= self.context_length and tuple(prompts_pseudo_tokens.shape) == tuple(x.shape[:2])
        return self._run(x, prompts_pseudo_tokens, shared_prefix_len if prompts_text is None else 0)

"""One optimizer step of the reference's training loop as ONE object (runner/vlsa_handler.py:260-289: 32 x ``net(X)``, ``torch.cat``,
``calc_objective_loss``, one ``backward``, ``optimizer.step``; cfg_vlsa_conch.yaml:111-118).

Why: the step is ~190 dependent kernel launches of 5-15 us (text tower forward + backward 150 of them) under 1.6-1.9 ms of Python -- host
and GPU are level, so neither a faster kernel nor a leaner host shows up alone.  ``TrainStep`` takes the host out of the
repeated case: the first time a batch -- the same bag tensors, the same label tensors -- comes, the step runs eagerly; the second time
it is captured into a hipGraph (``torch.cuda.CUDAGraph``: forward_bags, the fused loss kernel, the whole autograd backward and a
capturable Adam), and from then on the batch costs ONE host call.  Everything the kernels read is referenced by address (resident bags,
parameters, optimizer state, the label tensors), so replays see the parameters the previous step left.

What a replay cannot do is run Python: the in-place version counters of the parameters do not move.  ``step`` bumps them itself after
every replay (``torch._C._increment_version``), so every cache keyed on parameter versions (text features, prepared queries, look-ahead
windows: vlsa_amd/vlsa.py) misses exactly as after an eager ``optimizer.step()``.

Batches handed to ``step`` that never repeat (a sampler that reshuffles every epoch) stay eager -- same numbers, no capture.  For that
sampler there is ``set_epoch`` / ``step_next``: the bags stay in one resident ``BagSet``, the epoch's order goes to the device, and every
step begins with ONE launch (``vlsa_batch_gather``) that copies the next picks' descriptor rows and labels into slots at fixed addresses
(``functional.BagSlots``).  The step's launches read the slots, so ONE graph per batch size (the full batch, and the epoch's tail)
serves every batch: from the third step on a reshuffled run is replays.  ``graph=False`` disables capturing altogether.

Data parallel (``dist``): bags are the unit (SURVEY.md 8(e) "Training DP"); gradients are averaged with one all-reduce of a flat buffer
per step (eager steps only: a collective inside a captured step is left to the day a node exists).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from . import functional as VF


def _dbg(msg):
    if os.environ.get("VLSA_TRAINSTEP_DEBUG"):
        import sys
        sys.stderr.write(f"[TrainStep] {msg}\n")
        sys.stderr.flush()


def _bump_versions(tensors):
    try:
        torch._C._increment_version(tensors)            # torch >= 2.4: an iterable of tensors
    except (RuntimeError, TypeError):
        for t in tensors:
            torch._C._increment_version(t)


def _same_memory(a, b) -> bool:
    """the same label tensor as last epoch (the slots keep the one they read alive, so the same address and type is the same tensor)"""
    return a is b or (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.data_ptr() == b.data_ptr()
                      and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device)


class TrainStep:
    def __init__(self, net, objective, optimizer, dist=None, group=None, world: int = 1, graph: bool = True, max_graphs: int = 8,
                 capture_after: int = 1):
        self.net, self.objective, self.opt = net, objective, optimizer
        self.dist, self.group, self.world = dist, group, int(world)
        self.params = [p for g in optimizer.param_groups for p in g["params"]]
        from .losses import SurvObjective
        self._obj_takes_log = isinstance(objective, SurvObjective)
        self.graph_enabled = bool(graph) and self.world == 1 and self._capturable()
        self.max_graphs, self.capture_after = int(max_graphs), int(capture_after)
        self._seen = OrderedDict()          # batch key -> eager steps seen
        self._graphs = OrderedDict()        # batch key -> (graph, loss, kept)
        self._pool = None
        self._cap_stream = None
        self.why_eager: Optional[str] = None if self.graph_enabled else ("graph=False" if not graph else
                                                                        "data parallel" if self.world > 1 else "optimizer is not capturable")
        self.n_eager = self.n_replay = self.n_capture = 0
        self._epoch = None                  # set_epoch / step_next: the resident set, its slots and the device-side order
        self._why_slots: Optional[str] = None
        self._slot_replays = {"full": 0, "tail": 0}

    def _capturable(self) -> bool:
        return all(g.get("capturable", False) for g in self.opt.param_groups)

    # -- eager ------------------------------------------------------------------------------------------------------------------
    def _eager(self, bags, t, e, gather=None):
        """gather: the launch that refills ``bags`` (slots) in the stream -- part of the step, so a capture records it"""
        net = self.net
        if gather is not None:
            gather()
        logits = net.forward_bags(bags)[0]
        self.opt.zero_grad(set_to_none=True)
        if self._obj_takes_log and logits.dim() == 2 and logits.shape[0] <= 4096:
            # vlsa_amd.losses.SurvObjective: value AND gradient come out of its one launch (with the exp of the logit scale), so the
            # backward pass starts at the logits -- no ones_like seed, no product with the saved gradient (two launches of ~5 us)
            loss, g = self.objective.value_and_grad(logits, t, e, log_logit_scale=net.logit_scale)
            logits.backward(g)
        else:
            loss = self.objective(logits, t, e, net.get_logit_scale())
            loss.backward()
        if self.world > 1:
            self._allreduce_grads()
        self.opt.step()
        return loss.detach()          # (detached: a caller that keeps the loss must not keep the step's autograd graph -- and its
                                      #  AccumulateGrad nodes, bound to the stream they were created on -- alive into a capture)

    def _allreduce_grads(self):
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            return
        flat = torch.cat([g.reshape(-1) for g in grads])
        if self.dist.get_backend(self.group) != "nccl":
            host = flat.cpu()
            self.dist.all_reduce(host, group=self.group)
            flat.copy_(host)
        else:
            self.dist.all_reduce(flat, group=self.group)
        flat.div_(self.world)
        o = 0
        for g in grads:
            n = g.numel()
            g.copy_(flat[o:o + n].view_as(g))
            o += n

    # -- graph ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _key(bags, t, e):
        rows = bags.rows if isinstance(bags, VF.BagSet) else VF.bag_rows(bags)
        return (rows.tobytes(), t.data_ptr(), None if e is None else e.data_ptr(), t.shape)

    def _side(self, bags, t, e, gather=None):
        """one EAGER step on the capture stream (the step before a capture): whatever the step creates lazily -- allocator pools of
        that stream, autograd's per-parameter AccumulateGrad nodes, library handles -- then exists on the stream the capture runs on"""
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream()
        cur = torch.cuda.current_stream()
        self._cap_stream.wait_stream(cur)
        with torch.cuda.stream(self._cap_stream):
            loss = self._eager(bags, t, e, gather)
        cur.wait_stream(self._cap_stream)
        return loss

    def _capture(self, key, bags, t, e, gather=None):
        bagset = bags if isinstance(bags, VF.BagSet) else VF.BagSet(bags)
        bagset.desc()                                   # the descriptor table goes up outside the capture
        g = torch.cuda.CUDAGraph()
        self.opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        _dbg("capture begins")
        try:
            with torch.cuda.graph(g, pool=self._pool, stream=self._cap_stream,
                                  capture_error_mode=os.environ.get("VLSA_GRAPH_CAPTURE_MODE", "global")):
                loss = self._eager(bagset, t, e, gather)
        except Exception as exc:  # noqa: BLE001  (whatever refuses to be captured: this batch -- and the object -- stay eager)
            self.graph_enabled = False
            self.why_eager = f"capture failed: {type(exc).__name__}: {str(exc)[:300]}"
            _dbg(self.why_eager)
            try:
                torch.cuda.synchronize()
            except Exception:  # noqa: BLE001
                pass
            self.net._drop_text_cache()
            self.opt.zero_grad(set_to_none=True)
            return None
        _dbg("capture ended")
        if self._pool is None:
            self._pool = g.pool()
        self.n_capture += 1
        # a capture enqueues nothing: the step it recorded runs now
        self._graphs[key] = (g, loss, (bagset, t, e))
        while len(self._graphs) > self.max_graphs:
            self._graphs.popitem(last=False)
        return self._replay(key)

    def _replay(self, key):
        g, loss, _ = self._graphs[key]
        self._graphs.move_to_end(key)
        sync = getattr(self.opt, "sync_hyper", None)
        if sync is not None:
            sync()                                      # vlsa_amd.optim.FusedAdam: a changed learning rate reaches the device table
        g.replay()
        _bump_versions(self.params)                     # what optimizer.step() does to the version counters, without a kernel
        self.net._drop_text_cache()                     # (the capture left the text cache pointing at a graph-owned tensor)
        self.n_replay += 1
        return loss

    def step(self, bags: Sequence[torch.Tensor], t: torch.Tensor, e: Optional[torch.Tensor] = None):
        """bags: the step's resident bags (a list or a ``BagSet``); t / e: the labels on the device.  Returns the loss (a 0-dim device
        tensor; in graph mode the SAME tensor every time, overwritten by the next replay of that batch)."""
        if not self.graph_enabled:
            self.n_eager += 1
            return self._eager(bags, t, e)
        key = self._key(bags, t, e)
        if key in self._graphs:
            return self._replay(key)
        n = self._seen.get(key, 0)
        if n > self.capture_after:
            self._seen.pop(key, None)
            loss = self._capture(key, bags, t, e)
            if loss is not None:
                return loss
            self.n_eager += 1
            return self._eager(bags, t, e)
        self._seen[key] = n + 1
        if n == self.capture_after:         # the step before the capture: eager, on the capture stream
            while len(self._seen) > 4096:
                self._seen.popitem(last=False)
            self.n_eager += 1
            return self._side(bags, t, e)
        while len(self._seen) > 4096:
            self._seen.popitem(last=False)
        self.n_eager += 1
        return self._eager(bags, t, e)

    # -- an epoch over a resident set: batches drawn on the device ---------------------------------------------------------------
    def _slots_why_eager(self, slots) -> Optional[str]:
        """THE decision whether a step over ``BagSlots`` may be captured: None, or why not.  A graph over slots is replayed on bags of
        other sizes than it was captured on, so every launch of the route must take the sizes from the device table alone: the VLFAN
        training route (streaming forward + strided merge, ``head_train``, the objective, the persistent batch backward, the query
        chain, the text tower, the optimizer) with workspaces sized by (B, P, D).  The routes kept out size a buffer or a grid on the
        host: a Feat_Projecter in front and the DeepMIL / zero-shot encoders (by total rows), the bf16 backward for P > 12 (its partials
        by the largest bag), and poolings other than 'mean' (not the fused head)."""
        from .deepmil import VLFAN
        enc = getattr(self.net, "mil_encoder", None)
        if not isinstance(enc, VLFAN):
            return f"the {type(enc).__name__} encoder sizes its buffers by the batch's total rows"
        if enc.feat_proj is not None:
            return "the Feat_Projecter in front sizes its output by the batch's total rows"
        spec = enc.fused_head_spec()
        if spec is None or spec[0] != "mean":
            return "a query pooling other than 'mean' does not take the fused training head"
        if slots.dt != VF.nat.DT_F32 and int(enc.num_query) > 12:
            return "the bf16 backward for more than 12 queries sizes its partial sums by the batch's largest bag"
        return None

    def set_epoch(self, source, t_all: torch.Tensor, e_all: torch.Tensor, order, batch_size: int, groups: Optional[int] = None) -> None:
        """Begin an epoch over a resident set.  source: a ``BagSet`` of M bags; t_all [M] int64 / e_all [M] float32: its labels on the
        same device; order: the epoch's L picks (integers in [0, M): a permutation, or any other sampling), a sequence, numpy array or
        tensor; batch_size <= 64.  ``step_next`` then takes ``batch_size`` picks per step and, when ``L % batch_size`` is not zero, the
        rest as a last, smaller step -- the batches ``DataLoader(shuffle=True, drop_last=False)`` yields.
        The order is checked here, on the host (``ValueError``), and uploaded into a device buffer that is kept across epochs.  This is
        also where the epoch that just ended is looked at: ONE host sync per epoch reads the gather launches' status word and raises
        ``VlsaNativeError`` if any of them refused its picks (after the LAST epoch: ``check_epoch()``, or ``close()``).  Slots and their
        graphs are kept as long as source, labels, batch size, ``groups`` and L stay the same: L -- and with it the tail's size -- is a
        by-value argument of the captured gather launch, so an order of another length (a sampler of varying length) builds new slots
        and captures again.  groups: the slots' bags in flight (``BagSlots(groups=)``; the tail's slots take it capped at their own
        size); None: ``vlsa_batch_groups`` over a representative batch."""
        if not isinstance(source, VF.BagSet) or isinstance(source, VF.BagSlots):
            raise ValueError(f"set_epoch takes the resident bags as a BagSet, got {type(source).__name__}")
        M, batch_size = len(source), int(batch_size)
        if isinstance(order, torch.Tensor):
            order = order.detach().cpu().numpy()
        order = np.asarray(order)
        if order.dtype.kind not in "iu" or order.ndim != 1:
            raise ValueError(f"set_epoch: the order must be a 1-d sequence of integers, got dtype {order.dtype} with {order.ndim} dimension(s)")
        order = np.ascontiguousarray(order, dtype=np.int64)
        L = int(order.shape[0])
        if L < 1 or int(order.min()) < 0 or int(order.max()) >= M:
            raise ValueError(f"set_epoch: the order must hold at least one index, all in [0, {M}) (the source holds {M} bags)")
        if not (1 <= batch_size <= M):
            raise ValueError(f"set_epoch: batch_size {batch_size} outside [1, {M}] (the source holds {M} bags)")
        ep = self._epoch
        if ep is not None:
            self.check_epoch()
        dev = source[0].device
        groups = None if groups is None else int(groups)
        if not (ep is not None and ep["source"] is source and _same_memory(ep["t_all"], t_all) and _same_memory(ep["e_all"], e_all)
                and ep["batch"] == batch_size and ep["L"] == L and ep["groups"] == groups):
            # the slots' launches -- and their graphs -- have the label tensors, L and the order buffer's address baked in
            full = VF.BagSlots(source, batch_size, groups, t_all=t_all, e_all=e_all)
            n_tail = L % batch_size
            g_tail = None if groups is None else min(groups, 1 << (max(n_tail, 1).bit_length() - 1))     # a power of two <= n_tail
            tail = VF.BagSlots(source, n_tail, g_tail, t_all=t_all, e_all=e_all) if n_tail else None
            self._drop_slot_graphs()
            old = None if ep is None else ep["order"]
            buf = old if old is not None and old.device == dev and old.shape[0] >= L else torch.empty(L, dtype=torch.int64, device=dev)
            ep = self._epoch = {"source": source, "t_all": t_all, "e_all": e_all, "batch": batch_size, "L": L, "groups": groups, "order": buf,
                                "full": full, "tail": tail, "cursor": torch.zeros(1, dtype=torch.int64, device=dev),
                                "status": torch.zeros(1, dtype=torch.int32, device=dev)}
            self._why_slots = self._slots_why_eager(full)
        ep["order"][:L].copy_(torch.from_numpy(order))
        ep["cursor"].zero_()
        ep["host_order"], ep["pos"] = order, 0

    def check_epoch(self) -> None:
        """ONE host sync: raises ``VlsaNativeError`` if a gather launch since the last look refused its picks (it then left the slots
        on the previous batch, and that step trained on it once more).  ``set_epoch`` calls this for the epoch that ended."""
        ep = self._epoch
        if ep is None:
            return
        code = int(ep["status"].item())
        if code:
            ep["status"].zero_()
            what = {VF.nat.GATHER_BAD_CURSOR: "the cursor ran outside the order", VF.nat.GATHER_BAD_INDEX: "an index outside the source"}
            raise VF.nat.VlsaNativeError(f"vlsa_batch_gather refused a batch of the last epoch: {what.get(code, code)} (status {code})")

    def epoch_state(self) -> dict:
        """what the epoch's launches read and write: the ``BagSlots`` of the full batch and of the tail (or None), the device cursor
        (int64 [1]: picks consumed) and the gather launches' status word (int32 [1])"""
        ep = self._epoch
        if ep is None:
            raise RuntimeError("epoch_state() before set_epoch()")
        return {"full": ep["full"], "tail": ep["tail"], "cursor": ep["cursor"], "status": ep["status"]}

    def _drop_slot_graphs(self):
        for key in [k for k in list(self._graphs) + list(self._seen) if isinstance(k, tuple) and k and k[0] == "slots"]:
            self._graphs.pop(key, None)
            self._seen.pop(key, None)

    def step_next(self):
        """The next step of the epoch ``set_epoch`` began: ONE gather launch (the slots take the next picks, the device cursor moves
        on) and the step over the slots -- eager, eager on the capture stream, captured, or replayed as ``step`` does it for a batch
        that repeats, with the slots as the batch: the third step of a size is captured (the gather inside), every later one is ONE
        replay.  Returns the loss as ``step`` does; raises ``StopIteration`` when the order is consumed."""
        ep = self._epoch
        if ep is None:
            raise RuntimeError("step_next() before set_epoch()")
        pos, L = ep["pos"], ep["L"]
        if pos >= L:
            raise StopIteration("the epoch's order is consumed: set_epoch() begins the next one")
        kind = "full" if L - pos >= ep["batch"] else "tail"
        slots = ep[kind]
        idx = ep["host_order"][pos:pos + slots.batch]
        ep["pos"] = pos + slots.batch
        order, cursor, status = ep["order"], ep["cursor"], ep["status"]

        def gather():
            slots.gather(order, L, cursor, status)

        if not self.graph_enabled or self._why_slots is not None:
            slots.follow(idx)
            self.n_eager += 1
            return self._eager(slots, slots.t, slots.e, gather)
        key = ("slots", id(slots))                       # (the epoch keeps the slots alive for as long as the key is in use)
        if key in self._graphs:                         # the host's view is not consulted: the graph reads the device table
            self._slot_replays[kind] += 1
            return self._replay(key)
        slots.follow(idx)
        n = self._seen.get(key, 0)
        if n > self.capture_after:
            self._seen.pop(key, None)
            loss = self._capture(key, slots, slots.t, slots.e, gather)
            if loss is not None:
                self._slot_replays[kind] += 1
                return loss
            self.n_eager += 1                           # (a capture that failed enqueued nothing: the gather has not run yet)
            return self._eager(slots, slots.t, slots.e, gather)
        self._seen[key] = n + 1
        self.n_eager += 1
        if n == self.capture_after:
            return self._side(slots, slots.t, slots.e, gather)
        return self._eager(slots, slots.t, slots.e, gather)

    def describe(self) -> dict:
        d = {"mode": "hipGraph replay of the whole step" if self.n_replay else "eager", "eager_steps": self.n_eager,
             "captures": self.n_capture, "replays": self.n_replay, "why_eager": self.why_eager,
             "optimizer": type(self.opt).__name__ + ("(fused, capturable)" if self._capturable() else "")}
        if self._epoch is not None:
            d["slot_replays"] = dict(self._slot_replays)
            if d["why_eager"] is None and self._why_slots is not None:
                d["why_eager"] = "steps over slots stay eager: " + self._why_slots
        return d

    def close(self):
        """drops the graphs and the epoch; raises what ``check_epoch()`` raises for the last epoch (after everything is dropped)"""
        try:
            self.check_epoch()
        finally:
            self._graphs.clear()
            self._seen.clear()
            self._pool = None
            self._epoch = None

"""Drop-in counterpart of the reference's ``VLSA`` model (model/vlsa.py:21-198) for the per-bag forward.

What callers of the reference touch exists here with the same names and meaning:
``net(X) -> (logits[1,K], image_features, text_features)``, ``get_logit_scale()``, ``logit_scale``,
``mil_encoder`` (``VLFAN`` / ``FeatMIL`` / ``DeepMIL`` from ``vlsa_amd.deepmil``), ``forward_text_only()``,
``encode_instances()``, ``prompt_learner`` / ``prompt_encoder`` (whatever objects the caller plugs in -- the CONCH
text tower is out of scope and is consumed through ``text_provider``), and ``state_dict()`` keys
``logit_scale``, ``mil_encoder.visual_adapter.{weight,bias}``, ``mil_encoder.Q.residual_features`` ...

Text features are bag-independent; the reference re-runs its 12-layer text tower for every bag.
Here ``forward_text_only`` caches the provider's output keyed on the parameter versions of the provider, which is
exact: it is recomputed whenever an optimizer step (or any in-place update) touched those parameters.
"""
from __future__ import annotations

import math
import os
import random
from typing import Callable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import deepmil as mil_encoders
from . import functional as VF
from .deepmil import FeatMIL, VLFAN, logit_pooling
from .model_state import _HOOKS_INSTALLED, ModuleWatch, _install_structure_hooks     # noqa: F401  (re-exported: the tests read them here)


_PLAIN = frozenset((str, int, float, bool, type(None)))

# Invalidation levels of ``VLSA._invalidate`` -- the ONE statement of what each event clears:
#                                              _la   text cache   watches   _hot   _plans   _train_plans   _prepared_text / _query
#   _FORWARD  a differentiable forward          x
#   _WEIGHTS  load_state_dict                   x        x           x        x
#   _STORAGE  _apply (.to / .cuda / .float)     x        x           x        x       x          x                  x
_FORWARD, _WEIGHTS, _STORAGE = 0, 1, 2


def _env_flag(name: str) -> bool:
    return os.environ.get(name, "").strip().lower() not in ("", "0", "false", "no", "off")


# Environment-level switches for the stateful shortcuts of the boundary, read ONCE at import (a run is one way or the other):
#   VLSA_AMD_NO_DEFER=1      net(X) in training mode is never deferred (vlsa_amd/deferred.py), whatever `defer_training_calls` says
#   VLSA_AMD_NO_LOOKAHEAD=1  net(X) over ResidentBags items is never served from a look-ahead window (every call runs its own bag)
#   VLSA_AMD_PARANOID=1      every materialised deferred batch and every look-ahead window re-computes ONE random bag of it through
#                            the per-bag route and raises if the logits differ by more than 1e-4 (a device sync per batch / window)
ENV_NO_DEFER = _env_flag("VLSA_AMD_NO_DEFER")
ENV_NO_LOOKAHEAD = _env_flag("VLSA_AMD_NO_LOOKAHEAD")
ENV_PARANOID = _env_flag("VLSA_AMD_PARANOID")
ENV_NO_HOTCALL = _env_flag("VLSA_AMD_NO_HOTCALL")      # VLSA_AMD_NO_HOTCALL=1: every per-bag inference call takes the full route (round 6)
PARANOID_TOLERANCE = 1e-4


class ParanoidMismatch(RuntimeError):
    """VLSA_AMD_PARANOID=1: a batched shortcut (deferred training calls / look-ahead window) disagreed with the per-bag route."""


def build_mil_encoder(image_encoder_cfg: dict) -> nn.Module:
    """getattr(model.deepmil, cfg['name'])(**cfg)  (model/utils_vl.py:129-138)."""
    name = image_encoder_cfg["name"]
    if name == "DSMIL":
        # model/utils_vl.py builds it with num_cls = 2: its [1, 2] class logits cannot meet the [K, 512] text features of model/vlsa.py:185-192
        raise ValueError("Got an invalid MIL encoder name: DSMIL. As a VLSA image encoder DSMIL returns [1, num_cls] class logits, not a "
                         "[1, 512] visual feature that the text features could be compared with; it is served as the survival baseline "
                         "load_model('DeepMIL', dims, network='DSMIL') instead.")
    cls = getattr(mil_encoders, name, None)
    if cls is None or name.startswith("_"):
        raise ValueError(f"Got an invalid MIL encoder name: {name}.")
    return cls(**image_encoder_cfg)


def _encoder_extras(model):
    """the encoder watch's extras (a function of the model: no reference back to it): logit scale, plain-attribute co-attention scale"""
    cs = getattr(model._modules["mil_encoder"], "coattn_logit_scale", None)
    return [model._parameters["logit_scale"]] + ([cs] if isinstance(cs, torch.Tensor) else [])


class _ById:
    """stands for an object in a cache key: equal to another ``_ById`` of the SAME object only, and keeps the object alive"""
    __slots__ = ("obj",)

    def __init__(self, obj):
        self.obj = obj

    def __eq__(self, other):
        return other.__class__ is _ById and other.obj is self.obj

    def __hash__(self):
        return id(self.obj)


class _DeferredCoopFeatures:
    """Text features of a CoOp-pretrained, frozen prompt learner (model/vlsa.py:129-137) -- a tower pass that waits for the device.
    A plain object (picklable; deep copies of the model stay bound to their own encoder), see prompt_adapter._DeferredTowerPass."""

    def __init__(self, prompt_encoder, learner):
        self.prompt_encoder, self.learner = prompt_encoder, learner

    def __call__(self):
        dev = self.prompt_encoder.token_embedding.weight.device
        with torch.no_grad():
            return self.prompt_encoder(prompts_embedding=self.learner.to(dev)(), prompts_pseudo_tokens=self.learner.pseudo_sentence_tokens)


class VLSA(VF.nat.TransientCaches, nn.Module):
    """``VLSA(text_encoder_cfg, image_encoder_cfg, prompt_learner_cfg, pretrained_prompt_learner_cfg=None, vlsa_api=...,
    path_clip_model=...)`` -- the reference's constructor (model/vlsa.py:22-105), i.e. what ``load_model('VLSA', **arch_cfg)``
    calls from ``VLSAHandler.func_load_model`` (runner/vlsa_handler.py:112-120).  ``VLSA.from_modules(image_encoder_cfg, ...)``
    assembles the same model from ready-made parts (text features / provider / prompt learner + encoder objects)."""

    _transient = {"_hot": dict, "_plans": dict, "_train_plans": dict, "_watches": None, "_text_cache": lambda: None,
                  "_text_cache_key": lambda: None, "_prepared_text": lambda: None, "_prepared_query": lambda: None,
                  "_head_tickets": lambda: VF.HeadTickets(), "_la": lambda: None,
                  "_pending_calls": lambda: None, "_materialising": lambda: False, "_side_streams": None}

    #: bags per look-ahead window: an evaluation loop that calls ``net(X)`` once per bag of a ``vlsa_amd.ingest.ResidentBags`` dataset
    #: is served from ONE batched launch over the next bags of the dataset; 0 / 1 = off.  Windows of slide-sized bags grow beyond this
    #: -- up to 256 bags (one forward launch takes that many) as long as a window stays under ``lookahead_rows`` patch rows
    lookahead_bags = 64
    lookahead_rows = 3_200_000
    #: True: a grad-enabled ``net(X)`` in training mode is recorded, not run; the first torch operation on any of its outputs runs ONE
    #: ``forward_bags`` over all recorded bags (vlsa_amd/deferred.py) -- the reference handler's bag-by-bag training loop
    #: (runner/vlsa_handler.py:260-289) at the batched step's speed.  ``patch_reference()`` switches it on; off by default.
    defer_training_calls = False

    def __init__(self, text_encoder_cfg, image_encoder_cfg, prompt_learner_cfg, pretrained_prompt_learner_cfg=None,
                 info_prefix="VLSA-UNI", **kwargs):
        super().__init__()
        from . import hooks
        from .model_utils import get_prompt_encoder
        assert "vlsa_api" in kwargs, "Please specify `vlsa_api` in arguments."
        assert "path_clip_model" in kwargs, "Please specify `path_clip_model` in arguments."
        api, root = kwargs["vlsa_api"], kwargs["path_clip_model"]
        # host side (tokenizer, pretrained VL weights) through the hooks; model/vlsa.py:38-49
        self.text_tokenizer = hooks.make_tokenizer(root, text_encoder_cfg["name"], api)
        vl_model = hooks.load_vl_model(text_encoder_cfg, root, api)
        # language end (model/vlsa.py:51-70)
        self.pmt_learner_name = prompt_learner_cfg["name"]
        prompt_encoder = get_prompt_encoder(vl_model, api=api)
        self.prompt_encoder = prompt_encoder          # registered first: the builders below read it
        prompt_learner = text_module = None
        if self.pmt_learner_name == "CoOp":
            prompt_learner, frozen_features = self._build_prompt_learner(prompt_learner_cfg, pretrained_prompt_learner_cfg)
        elif self.pmt_learner_name == "Adapter":
            text_module, frozen_features = self._build_prompt_adapter(prompt_learner_cfg, pretrained_prompt_learner_cfg), False
        else:
            raise ValueError(f"{self.pmt_learner_name} is not a valid name of prompt learner.")
        # vision end + the query network of VLFAN (model/vlsa.py:72-99)
        query_network = None
        if image_encoder_cfg["name"] == "VLFAN" and image_encoder_cfg["query"] == "Text":
            qcfg = {k[len("query_text_"):]: v for k, v in image_encoder_cfg.items() if k.startswith("query_text_")}
            qcfg.update(tokenizer=self.text_tokenizer, num_prompts=image_encoder_cfg["num_query"],
                        load_negative_prompts=image_encoder_cfg.get("gated_query", False))
            from .model_utils import load_prompt_adapter
            query_network = load_prompt_adapter(prompt_encoder, qcfg)
        self.text_encoder_cfg, self.prompt_learner_cfg = text_encoder_cfg, prompt_learner_cfg
        self._assemble(image_encoder_cfg, text_provider=text_module, query_network=query_network, prompt_learner=prompt_learner,
                       prompt_encoder=prompt_encoder, logit_scale=vl_model.logit_scale, kwargs=kwargs,
                       frozen_coop_features=bool(frozen_features))
        self.image_encoder_cfg = image_encoder_cfg      # the caller's dict object, as in the reference (model/vlsa.py:102)

    @classmethod
    def from_modules(cls, image_encoder_cfg: dict, text_provider: Optional[Callable[[], torch.Tensor]] = None,
                     pretrained_text_features: Optional[torch.Tensor] = None, query_network: Optional[nn.Module] = None,
                     logit_scale_init: float = math.log(1 / 0.07), prompt_learner: Optional[nn.Module] = None,
                     prompt_encoder: Optional[nn.Module] = None, cache_text_features: bool = True, **kwargs):
        """image_encoder_cfg: the ``vlsa_img_encoder_*`` keys of cfg_vlsa_conch.yaml with the prefix stripped
        (runner/vlsa_handler.py:110-111).  Text side: ``pretrained_text_features`` [K, D] (the reference's cached
        branch, model/vlsa.py:160-161) or ``text_provider`` -- any callable returning [K, D], e.g. the reference's
        ``lambda: prompt_encoder(prompts_embedding=prompt_learner(), prompts_pseudo_tokens=...)`` -- or a
        ``prompt_learner`` + ``prompt_encoder`` pair (the CoOp route on the device)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._assemble(image_encoder_cfg, text_provider=text_provider, pretrained_text_features=pretrained_text_features,
                       query_network=query_network, prompt_learner=prompt_learner, prompt_encoder=prompt_encoder,
                       logit_scale=logit_scale_init, cache_text_features=cache_text_features, kwargs=kwargs)
        return self

    def _assemble(self, image_encoder_cfg, text_provider=None, pretrained_text_features=None, query_network=None,
                  prompt_learner=None, prompt_encoder=None, logit_scale=math.log(1 / 0.07), cache_text_features=True, kwargs=None,
                  frozen_coop_features=False):
        _install_structure_hooks()      # process-global registration hooks (vlsa_amd/model_state.py): only once a VLSA model exists
        self.kwargs = kwargs or {}
        self.image_encoder_cfg = dict(image_encoder_cfg)
        self.mil_encoder = build_mil_encoder(self.image_encoder_cfg)
        if isinstance(self.mil_encoder, VLFAN) and self.mil_encoder.query_type == "Text":
            if query_network is None:
                raise ValueError("VLFAN(query='Text') needs `query_network` (e.g. vlsa_amd.prompt_adapter.PromptAdapter)")
            self.mil_encoder.reset_query(query_network)
        if pretrained_text_features is not None:
            self.register_buffer("pretrained_text_features", pretrained_text_features.detach().clone(), persistent=False)
        elif frozen_coop_features:
            # pretrained + fully frozen CoOp prompts: the reference pre-computes the text features in its constructor and
            # never runs the tower again (model/vlsa.py:57-60,117-122).  The HIP tower needs the device, and the handler moves
            # the model there only after construction: the buffer exists from the start (``hasattr`` is the reference's
            # switch, model/vlsa.py:160) and is filled by the first ``forward_text_only``.
            self.register_buffer("pretrained_text_features", None, persistent=False)
        if prompt_learner is not None:
            self.prompt_learner = prompt_learner
        if prompt_encoder is not None:
            self.prompt_encoder = prompt_encoder
        if (text_provider is None and pretrained_text_features is None and prompt_learner is not None
                and prompt_encoder is not None):
            # the reference's CoOp route (model/vlsa.py:149-156,163-164): rank prompts -> text tower, both on the GPU here
            text_provider = self._coop_text_features
        # An nn.Module given as the provider IS the reference's 'Adapter' prompt learner (model/vlsa.py:65-66,166-167): it is
        # registered under the reference's attribute name so that checkpoints carry `prompt_adapter.*` keys.
        self._provider_is_module = isinstance(text_provider, nn.Module)
        if self._provider_is_module:
            self.prompt_adapter = text_provider
            self.text_provider = None
        else:
            self.text_provider = text_provider
        self.cache_text_features = cache_text_features
        self._drop_text_cache()
        if isinstance(logit_scale, nn.Parameter):
            self.logit_scale = logit_scale             # the VL model's own parameter (model/vlsa.py:105)
        else:
            self.logit_scale = nn.Parameter(torch.ones([]) * float(logit_scale))  # CoCa init, model/conch/coca_model.py:187
        self._plans = {}
        self._hot = {}                 # (D, dtype, device) -> (eval state, pre-built per-bag call, row stride): see _fused_vlfan
        self._train_plans = {}
        self._la = None                                        # look-ahead window (see _lookahead)
        self._pending_calls, self._materialising = None, False  # deferred training calls (vlsa_amd/deferred.py)
        self._head_tickets = VF.HeadTickets()
        self._prepared_text, self._prepared_gen = None, 0     # see _fused_vlfan: what the plans' prepared T^ / queries were computed from
        self._prepared_query, self._prepared_qver = None, -1

    # -- builders of the text side (model/vlsa.py:107-147) -----------------------------------------------------------------
    def _build_prompt_learner(self, prompt_learner_cfg, pretrained_prompt_learner_cfg):
        """-> (prompt learner, whether its text features are fixed for good).  CoOp learner over this model's tokenizer and the
        tower's token embedding; with ``pretrained`` its embeddings come from a checkpoint, and when both are frozen as well
        the text features never change again."""
        from .model_utils import load_prompt_learner
        cfg = dict(prompt_learner_cfg)
        cfg.update(tokenizer=self.text_tokenizer, text_config=self.prompt_encoder.text_config,
                   token_embedding=self.prompt_encoder.token_embedding)
        learner = load_prompt_learner(cfg["method"], cfg)
        fixed = False
        if cfg["pretrained"]:
            assert pretrained_prompt_learner_cfg is not None, "Please specify `config` for `pretrained_prompt_learner`."
            learner.load_pretrained_parameters(pretrained_prompt_learner_cfg["ckpt"])
            fixed = bool(cfg["frozen_context_embeds"] and cfg["frozen_rank_embeds"])
        return learner, fixed

    def _build_prompt_adapter(self, prompt_learner_cfg, pretrained_prompt_learner_cfg):
        """Text-side 'Adapter' learner (model/vlsa.py:124-147): a PromptAdapter over the rank sentences, or -- ``pretrained`` --
        over the text features of a CoOp-pretrained, frozen prompt learner."""
        from .model_utils import load_prompt_adapter
        cfg = dict(prompt_learner_cfg)
        features = None
        if cfg["pretrained"]:
            coop_cfg = dict(pretrained_prompt_learner_cfg)
            coop_cfg["pretrained"] = True
            learner, fixed = self._build_prompt_learner(coop_cfg, {"ckpt": coop_cfg["ckpt"]})
            assert fixed, "Found empty `pretrained_text_features`."
            features = _DeferredCoopFeatures(self.prompt_encoder, learner)     # evaluated once the tower is on the device
        cfg.update(tokenizer=self.text_tokenizer, num_prompts=cfg["num_ranks"], pretrained_prompt_features=features)
        return load_prompt_adapter(self.prompt_encoder, cfg)

    # -- model state: one kept walk per provider module and one for the MIL encoder (vlsa_amd/model_state.py states the rules), the
    #    keys of the text cache, of the look-ahead / hot call and of the deferred training calls over them, and what clears what ------
    _PROVIDER_NAMES = ("prompt_learner", "prompt_encoder", "prompt_adapter")

    def _providers(self):
        mods = self._modules
        return [(n, mods[n]) for n in self._PROVIDER_NAMES if mods.get(n) is not None]

    def _get_watches(self):
        """the watches, made on use: a deep copy / pickle drops them, and a model pickled before they existed has none"""
        ws = self.__dict__.get("_watches")
        if ws is None:
            ws = self.__dict__["_watches"] = {n: ModuleWatch() for n in self._PROVIDER_NAMES}
            ws["mil_encoder"] = ModuleWatch(_encoder_extras)
        return ws

    def _provider_key(self, exact=False):
        """Everything the provider's output depends on that this object can see: the grad mode + the stamp of every provider module
        (identity + in-place version of every parameter and buffer, the train / eval flag of every submodule: dropout in the 'FC'
        adapter).  None = the provider is an opaque callable with no declared modules: its output cannot be cached.  The reference's
        handler calls the model once per bag, so this runs per bag: in steady state nothing is walked."""
        mods = self._providers()
        if not mods:
            return None
        ws = self.__dict__.get("_watches") or self._get_watches()
        return (torch.is_grad_enabled(), *[ws[n].stamp(m, exact) for n, m in mods])

    #: plain (non-tensor) attributes of the MIL encoder that change what a forward computes: part of the look-ahead / deferral state
    _ENC_SCALAR_NAMES = ("keep_ratio", "pooling", "query_pooling", "gated_query", "pred_head", "query_type")

    def _eval_state(self, text_features=None, exact=False):
        """Everything an inference result depends on besides the bag, as (encoder part, version of the text features, the text-feature
        tensor): the text side's own cache hands out the same tensor object as long as ITS key holds.  The encoder part (hashable; all
        that ``_defer_key`` takes, without text features) = the stamp of the MIL encoder's watch -- its tensors and flags, the logit
        scale, the co-attention scale --, the plain attributes of ``_ENC_SCALAR_NAMES`` as this INSTANCE carries them and the
        zero-shot pooling spec.  The attributes are read from the encoder's ``__dict__``: a name held as a Parameter / submodule
        (``query_pooling``) is not there, it is in the watch's lists; a value that is no plain scalar enters by its identity (``_ById``
        keeps it alive).  ``exact``: walk the encoder again (a window is computed, a deferred batch opened)."""
        enc = self._modules["mil_encoder"]
        vals = tuple(map(enc.__dict__.get, self._ENC_SCALAR_NAMES))
        if not _PLAIN.issuperset(map(type, vals)):
            vals = tuple(v if v.__class__ in _PLAIN else _ById(v) for v in vals)
        watch = (self.__dict__.get("_watches") or self._get_watches())["mil_encoder"]
        encoder_part = (watch.stamp(enc, exact, self), vals, self.image_encoder_cfg.get("pooling"))
        return encoder_part, None if text_features is None else text_features._version, text_features

    @staticmethod
    def _same_state(a, b):
        return a[0] == b[0] and a[1] == b[1] and a[2] is b[2]

    def _defer_key(self, exact=False):
        """Everything a training-mode output depends on besides the bag: the text side (fixed features: the buffer -- by identity,
        kept alive -- and its version; a provider: ``_provider_key``), the encoder part of ``_eval_state``, ``self.training``.  None: a
        text provider this object cannot see into -- such calls are not deferred.  ``exact``: walk the encoder again (a new batch)."""
        fixed = self._buffers.get("pretrained_text_features")
        text = self._provider_key() if fixed is None else (_ById(fixed), fixed._version)
        return None if text is None else (text, self._eval_state(None, exact)[0], self.training)      # [0]: the encoder part

    def _invalidate(self, level):
        """drop what an event of ``level`` makes stale: the table at ``_FORWARD`` / ``_WEIGHTS`` / ``_STORAGE``"""
        self._la = None
        if level >= _WEIGHTS:
            self._drop_text_cache()
            for w in self._get_watches().values():
                w.forget()
            self._hot.clear()
        if level >= _STORAGE:
            self._plans.clear()
            self._train_plans.clear()
            self._prepared_text = self._prepared_query = None

    # -- text side -----------------------------------------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float(): tensors change under the same Parameter objects and versions -- nothing cached survives
        if "_plans" in self.__dict__:            # (not yet there when a parent converts a half-built model)
            self._invalidate(_STORAGE)
        out = super()._apply(fn, *args, **kwargs)
        self._materialise_frozen_prototypes()
        return out

    def _materialise_frozen_prototypes(self):
        """The reference computes its frozen text prototypes in the constructors, from the PRETRAINED tower (model/vlsa.py:57-60,
        prompt_adapter.py:60-79).  Here those tower passes wait for the device -- and run as soon as the model arrives there
        (this is called at the end of ``_apply``, i.e. of ``.cuda()`` / ``.to(device)``), before a later ``load_state_dict`` could
        put trained tower weights under them."""
        if "_plans" not in self.__dict__:
            return
        tower = getattr(self, "prompt_encoder", None)
        tensors = getattr(tower, "_tower_tensors", None)
        if tensors is None or not tensors()[0].is_cuda:
            return
        from .prompt_adapter import PromptAdapter
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, PromptAdapter) and m.pending_on_device():
                    m._materialise()
            if self._buffers.get("pretrained_text_features", 0) is None and getattr(self, "prompt_learner", None) is not None:
                self._fixed_text_features()

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        if "_plans" in self.__dict__:
            self._invalidate(_WEIGHTS)
        return out

    def compute_text_features_with_coop(self, prompt_learner):
        """prompt learner's sentence embeddings through the text tower (model/vlsa.py:149-156)."""
        from .prompt_encoder import HipTextTower
        extra = {}
        if isinstance(self.prompt_encoder, HipTextTower):      # the HIP tower evaluates the sentences' shared prefix once
            extra["shared_prefix_len"] = int(getattr(prompt_learner, "shared_prefix_len", 0) or 0)
        return self.prompt_encoder(prompts_embedding=prompt_learner(),
                                   prompts_pseudo_tokens=prompt_learner.pseudo_sentence_tokens, **extra)

    def _coop_text_features(self):
        return self.compute_text_features_with_coop(self.prompt_learner)

    def _drop_text_cache(self, *_):
        self._text_cache = self._text_cache_key = None

    def _fixed_text_features(self):
        """The ``pretrained_text_features`` buffer, or None when this model has none.  A buffer registered empty (pretrained,
        fully frozen CoOp prompts built before the model was on the device) is filled by its one tower pass here."""
        if "pretrained_text_features" not in self._buffers:
            return None
        t = self._buffers["pretrained_text_features"]
        if t is None:
            with torch.no_grad():
                t = self.compute_text_features_with_coop(self.prompt_learner).detach().clone()
            self._buffers["pretrained_text_features"] = t
        return t

    def forward_text_only(self):
        fixed = self._fixed_text_features()
        if fixed is not None:
            return fixed.clone()
        provider = self.prompt_adapter if self._provider_is_module else self.text_provider
        if provider is None:
            raise RuntimeError("no text features: give `pretrained_text_features` or `text_provider`")
        key = self._provider_key() if self.cache_text_features else None
        if key is None:
            return provider()
        if self._text_cache is None or key != self._text_cache_key:
            key = self._provider_key(exact=True)     # a miss re-walks the providers: a swapped parameter object is seen here at the latest
            feats = provider()
            if feats.requires_grad and feats.grad_fn is not None:
                # the cached tensor carries the provider's autograd graph: every bag of the step may hang off it, but once
                # a backward pass has run through it the graph is gone -- the next forward must rebuild it (per-bag
                # backward, gradient accumulation) even though no parameter has changed yet
                feats.register_hook(self._drop_text_cache)
            self._text_cache, self._text_cache_key = feats, key
        return self._text_cache

    def _text_features(self):
        """forward_text_only without the defensive clone of the cached-features branch (nothing here writes to it)."""
        fixed = self._fixed_text_features()
        return fixed if fixed is not None else self.forward_text_only()

    def encode_instances(self, X):
        return self.mil_encoder(X)

    def get_logit_scale(self):
        return self.logit_scale.exp()

    # -- forward -----------------------------------------------------------------------------------------
    def _needs_grad(self, text_features):
        if not torch.is_grad_enabled():
            return False
        # the text side reaches the output through `text_features` only, so its parameters need no look: what is left are the
        # logit scale and the MIL encoder (a walk over the whole model -- 150 tower tensors first -- cost ~0.3 ms per bag with
        # frozen prompts, in the loop that calls the model once per bag)
        if text_features.requires_grad or self.logit_scale.requires_grad:
            return True
        return any(p.requires_grad for p in self.mil_encoder.parameters())

    def _fused_vlfan(self, X, text_features):
        # Round 6, the hot call: the SAME model state and a bag of a shape seen before -> one pre-built C call (see
        # ``VlfanInferencePlan.hot_call``).  "Same state" is the look-ahead's definition (``_eval_state``: identity + in-place version of
        # every encoder tensor, the logit scale, the text-feature tensor, train / eval flags, the plain attributes); an entry is
        # rewritten by every slow-path call of its plan, so its state is the one the plan's prepared block was computed under.
        hot = self._hot
        if hot and not ENV_NO_HOTCALL and type(X) is torch.Tensor and X.dim() == 3:
            ent = hot.get((X.shape[2], X.dtype, X.device))           # (any bag size: the plan behind it takes N from the bag)
            if (ent is not None and X.shape[0] == 1 and X.shape[1] > 0 and X.stride(2) == 1 and X.stride(1) == ent[2]
                    and (X.data_ptr() & 15) == 0
                    and self._same_state(ent[0], self._eval_state(text_features))):
                return ent[1](X)
        enc = self.mil_encoder
        spec = enc.fused_head_spec() if isinstance(enc, VLFAN) else None
        if spec is None or X.dim() != 3 or X.shape[0] != 1 or not X.is_cuda or X.shape[1] == 0:
            return None
        X = enc.project(X)          # use_feat_proj=True: the fused Feat_Projecter launch first (no grad is needed here)
        mode, pw, W, b = spec
        X2 = VF._bag2d(X)
        N, D = X2.shape
        Qsrc = enc.step_query()                     # a text adapter's output is evaluated once per parameter version, not per bag
        P = Qsrc.shape[0] - (1 if enc.gated_query else 0)
        K = text_features.shape[0]
        if not (1 <= P <= 16 and 1 <= K <= 64 and D % 8 == 0 and D <= 1024):
            return None
        key = (None, D, P, K, X2.dtype, X2.device, enc.gated_query, mode, W is None)     # one plan for every bag size (round 6)
        plan = self._plans.get(key)
        qmod = pw if mode == "module" else None
        if qmod is not None:
            pw = None
        if plan is None:
            if len(self._plans) > 64:
                self._plans.clear()
                self._hot.clear()
            plan = VF.VlfanInferencePlan(None, D, P, K, X2.device, gated=enc.gated_query, pool="mean" if qmod is not None else mode,
                                         identity_head=W is None, coattn_scale=float(enc.coattn_logit_scale.exp()))
            self._plans[key] = plan
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=X2.device)  # noqa: E731
        outs = {"logits": f(1, K), "vhat": f(1, D), "That": None}   # fresh tensors, written by the kernels directly
        # queries / text features only change with their parameters: in an evaluation loop they are prepared once, not per bag.
        # The key never contains the ADDRESS of a transient tensor (a freed block is handed out again by the caching allocator
        # with `_version == 0`): the text side contributes the identity of the exact tensor object the last preparation read,
        # which this module keeps alive (`_prepared_text`), the queries likewise (`_prepared_query`: the tensor `step_query` hands
        # out, whose own cache follows the query network's parameters).  A query source that is a plain callable gives no key:
        # prepare every call.
        pkey = self._params_key(enc, Qsrc, text_features)
        Q, Tc, lsc, Wc, bc, pwc = self._f32_operands(Qsrc, text_features, W, b, pw)
        plan.run(X2, Q, Tc, lsc, Wc, bc, pwc, outs=outs, params_key=pkey, query_pool_module=qmod)
        sq = enc.__dict__.get("_step_query")
        shared_query = isinstance(enc.Q, torch.Tensor) or (sq is not None and sq[1] is Qsrc)     # (a stochastic query network -- active
        if (pkey is not None and shared_query and qmod is None and enc.feat_proj is None          #  dropout -- is evaluated per call)
                and X2.stride(1) == 1 and (X2.data_ptr() & 15) == 0
                and X2.dtype in (torch.float32, torch.bfloat16) and plan.scores is None):
            # the next bag of this shape under this state: the pre-built call (the prepared block of `plan` now belongs to this state)
            if len(self._hot) > 64:
                self._hot.clear()
            self._hot[(D, X2.dtype, X2.device)] = (self._eval_state(text_features),
                                                     plan.hot_call(Tc, lsc, Wc, bc, pwc, outs["That"]), X2.stride(0))
        else:
            self._hot.pop((D, X2.dtype, X2.device), None)
        return outs["logits"], outs["vhat"], outs["That"]

    def _f32_operands(self, Qsrc, text_features, W, b, pw):
        """(Q, T, logit scale, W, b, pool weights) as the fused kernels read them: detached, fp32, contiguous; None stays None"""
        def f32(t):        # (.float() / .contiguous() hand back the tensor itself when there is nothing to convert)
            return None if t is None else t.detach().float().contiguous()
        return (f32(Qsrc), f32(text_features), self.logit_scale.detach().float(), f32(W), f32(b),
                None if pw is None else pw.detach().float().reshape(-1).contiguous())

    def _params_key(self, enc, Qsrc, text_features):
        """Key of the (queries, text features) a plan's prepared block was computed from, or None = prepare every call (a query source
        that is a plain callable gives a fresh tensor per call: nothing to key on).  ``step_query`` hands out the SAME tensor object as
        long as the query source's parameters / buffers, flags and the grad mode are unchanged (a Parameter query: the parameter
        itself), so identity + in-place version of that object -- kept alive here -- is the query part of the key; the text side
        contributes the identity of the exact tensor object the last preparation read (``_prepared_text``) + its version.  Never the
        ADDRESS of a transient tensor: a freed block is handed out again by the caching allocator with ``_version == 0``."""
        if not isinstance(enc.Q, (nn.Module, torch.Tensor)):
            return None
        if self._prepared_text is not text_features or self._prepared_query is not Qsrc or self._prepared_qver != Qsrc._version:
            self._prepared_text, self._prepared_query, self._prepared_qver = text_features, Qsrc, Qsrc._version
            self._prepared_gen += 1
        return (self._prepared_gen, text_features._version)

    def _slide_train(self, X, text_features):
        """One bag with a gradient needed, VLFAN encoder with mean query pooling and a Linear / identity adapter (the shipped
        configuration): ONE autograd node per bag over the HIP forward / backward (``VF.slide_train``).  The reference's handler
        trains bag by bag (runner/vlsa_handler.py:267-289) and that loop is host-bound.  None: no such form (the general
        route follows)."""
        enc = self.mil_encoder
        if (not isinstance(enc, VLFAN) or not isinstance(X, torch.Tensor) or X.dim() != 3 or X.shape[0] != 1 or not X.is_cuda
                or X.requires_grad or X.shape[1] == 0):
            return None
        spec = enc.fused_head_spec()
        if spec is None or spec[0] != "mean":
            return None
        if enc.feat_proj is not None:
            if enc._projecter_trains():
                X = enc.project(X)              # its own HIP autograd node; the aggregation node below hands dX back to it
                if not (X.is_cuda and X.dtype == torch.float32 and X.shape[-1] == 512):
                    return None
            else:
                with torch.no_grad():
                    X = enc.project(X)
        X2 = VF._bag2d(X)
        N, D = X2.shape
        T = text_features
        if (D != 512 or X2.dtype not in (torch.float32, torch.bfloat16) or not T.is_cuda or T.dim() != 2 or T.shape[1] != D
                or not (1 <= T.shape[0] <= 64)):
            return None
        Q = enc.step_query()
        if not isinstance(Q, torch.Tensor) or Q.dim() != 2 or Q.shape[1] != D or not Q.is_cuda:
            return None
        P = Q.shape[0] - (1 if enc.gated_query else 0)
        W, b = spec[2], spec[3]
        ls = self.logit_scale
        if not (1 <= P <= VF.nat.MAX_P) or ls.dtype != torch.float32 or not ls.is_cuda:
            return None
        if W is not None and (W.dtype != torch.float32 or not W.is_contiguous() or tuple(W.shape) != (D, D) or not W.is_cuda
                              or (b is not None and (b.dtype != torch.float32 or not b.is_contiguous()))):
            return None
        K = T.shape[0]
        scale = enc.coattn_scale()
        key = (D, P, K, X2.device, enc.gated_query, W is None, scale)
        plan = self._train_plans.get(key)
        if plan is None:
            if len(self._train_plans) > 8:
                self._train_plans.clear()
            plan = self._train_plans[key] = VF.SlideTrainPlan(D, P, K, X2.device, enc.gated_query, W is None, scale)
        # fp32-contiguous Q / T: converted once per step, not per bag (the flat parameter tensor is keyed on tensor identity)
        return VF.slide_train(X2, plan.f32c("Q", Q), W, b, plan.f32c("T", T), ls, plan)

    def forward(self, X):
        """X: [1, N, D] bag -> (logits [1, K], image_features (unit-norm), text_features (unit-norm)).
        A list / tuple of bags is routed to ``forward_bags`` (so that wrappers which only hook ``forward`` --
        ``DistributedDataParallel`` with bags as the data-parallel unit -- see the batched path too)."""
        if isinstance(X, (list, tuple)):
            return self.forward_bags(list(X))
        la = self._la
        if la is not None and la["rows"] and not self.training and not torch.is_grad_enabled():
            # the evaluation loop's common case first -- a call that a look-ahead window already holds the answer for (the exact item,
            # then the exact model state: `_lookahead_hit`) -- before anything a miss needs is computed
            src = getattr(X, "_vlsa_src", None)
            if src is not None and src[0] is la["rb"] and not ENV_NO_LOOKAHEAD and not self._materialising and self.lookahead_bags > 1:
                hit = self._lookahead_hit(la, src[1], X)
                if hit is not None:
                    return hit
        pc = self._pending_calls
        if (pc is not None and self.defer_training_calls and not ENV_NO_DEFER and not self._materialising and self.training
                and torch.is_grad_enabled()):
            # a further call of an open batch of deferred training calls (vlsa_amd/deferred.py): nothing to evaluate here
            if type(X) is not torch.Tensor and isinstance(X, torch.Tensor):
                with torch._C.DisableTorchFunctionSubclass():      # a tagged resident view: every attribute read below would dispatch
                    X = X.as_subclass(torch.Tensor)
            if pc.same_state() and pc.takes(X):
                return pc.add(X)
        src = getattr(X, "_vlsa_src", None)          # a ResidentBags item as the handler's loader delivers it (vlsa_amd/ingest.py)
        text_features = self._text_features()
        needs_grad = self._needs_grad(text_features)
        if src is not None:
            if not needs_grad and not self.training and self.lookahead_bags > 1 and not ENV_NO_LOOKAHEAD and not self._materialising:
                ahead = self._lookahead(src, X, text_features)
                if ahead is not None:
                    return ahead
            X = X.as_subclass(torch.Tensor)
        if not needs_grad:
            fused = self._fused_vlfan(X, text_features)
            if fused is not None:
                return fused
        else:
            self._invalidate(_FORWARD)           # a differentiable forward: parameters are about to move
            if self.defer_training_calls and not ENV_NO_DEFER and self.training and not self._materialising:
                deferred = self._defer_call(X, text_features)
                if deferred is not None:
                    return deferred
            trained = self._slide_train(X, text_features)
            if trained is not None:
                return trained
        enc = self.mil_encoder
        if (isinstance(enc, FeatMIL) and enc.pooling not in ("mean", "max")
                and not (torch.is_grad_enabled() and (text_features.requires_grad or X.requires_grad))):
            return self._forward_zeroshot(X, text_features)      # inference: fused HIP route (nothing to differentiate)
        feats = self.encode_instances(X)
        if (not self._needs_grad(text_features) and feats.is_cuda and feats.dim() == 2 and feats.shape[0] == 1
                and feats.shape[1] % 4 == 0 and feats.shape[1] <= 1024 and text_features.shape[0] <= 64):
            # any encoder, no gradient: normalise + cosine logits of the bag vector in the head kernel (2 launches instead of
            # ~8 torch ops; these paths are host-bound)
            That, _ = VF.normalize_rows(text_features.detach())
            h = VF.head_forward(feats, "given", None, None, None, That, self.logit_scale.detach())
            return h["logits"][None, :], h["vhat"][None, :], That
        if feats.dim() == 2 and feats.shape[0] == 1 and self._train_head_takes(feats, text_features):
            # any encoder, gradient needed: both normalisations and the cosine logits as ONE autograd node (two launches each way:
            # the batched training head with B = P = 1 and an identity adapter) instead of ~12 torch ops and as many backward
            # nodes -- the bag-by-bag training loop is bound by those
            return VF.head_train(feats[None], None, None, text_features, self.logit_scale, self._head_tickets)
        text_features = F.normalize(text_features, dim=-1)
        image_features = F.normalize(feats.float(), dim=-1)
        logits = self.logit_scale.exp() * image_features @ text_features.t()
        if logits.shape[0] > 1:
            _, logits = logit_pooling(logits, self.image_encoder_cfg["pooling"])
        return logits, image_features, text_features

    # -- deferred training calls: the reference handler's bag-by-bag TRAINING loop at batched speed (vlsa_amd/deferred.py) -------
    def _defer_call(self, X, text_features):
        from .deferred import TrainingCalls
        if not (TrainingCalls.takes(X) and text_features.dim() == 2):
            return None
        enc = self.mil_encoder
        if isinstance(enc, FeatMIL) and enc.pooling not in ("mean", "max"):
            # identity FeatMIL (zero-shot logit pooling with trainable prompts): the per-bag call returns the bag's [N, D] patch
            # features as its second output (model/vlsa.py:188-196) -- a deferred batch hands out ONE row per bag, so per-bag calls run
            # as they come, through torch ops.  The batched HIP route of this stage is ``forward_bags`` (``_forward_bags_zeroshot_train``).
            return None
        if not isinstance(enc, (VLFAN, FeatMIL, mil_encoders.DeepMIL)):
            return None                                      # an encoder this package does not know: no claim about its output shape
        pc = self._pending_calls
        if pc is None or not pc.same_state():
            key = self._defer_key(exact=True)                # an exact walk of the encoder for the batch's key
            if key is None:
                return None
            # every module / tensor of the model from the walks the key was just built from (the encoder's watch; the providers'
            # when the text side runs per step) -- no second walk over the ~120 modules of the tower
            ws = self._get_watches()
            names = ["mil_encoder"] + ([n for n, _ in self._providers()] if self._buffers.get("pretrained_text_features") is None else [])
            sub, tensors = [x for n in names for x in ws[n].lists()[0]], [t for n in names for t in ws[n].lists()[1]]
            if any(isinstance(m, nn.modules.dropout._DropoutNd) and m.p > 0 and m.training for m in sub):
                return None                                  # per-call random masks: every call is its own evaluation
            pc = self._pending_calls = TrainingCalls(self, key, [t for t in tensors if t.requires_grad], text_features.shape[0],
                                                     text_features.shape[1], X.device)
        return pc.add(X)

    # -- VLSA_AMD_PARANOID=1: cross-check of the batched shortcuts against the per-bag route ----------------------------------------
    def _paranoid_check(self, X, logits_row, what: str):
        """Re-compute ONE bag of a deferred batch / look-ahead window through the per-bag route (``forward`` under ``no_grad`` with
        deferral and look-ahead off: the single-bag kernels) and compare the logits at ``PARANOID_TOLERANCE``; raises
        ``ParanoidMismatch``.  Syncs the device: a debug mode."""
        prev, la, pending = self._materialising, self._la, self._pending_calls
        self._materialising = True
        try:
            with torch.no_grad():
                Xp = X.as_subclass(torch.Tensor) if type(X) is not torch.Tensor else X
                ref = self.forward(Xp if Xp.dim() == 3 else Xp[None])[0]
        finally:
            self._materialising, self._la, self._pending_calls = prev, la, pending
        ref = ref.detach().float().reshape(-1)
        err = float((ref - logits_row.detach().float().reshape(-1)).abs().max())
        # the logits scale with exp(logit_scale), which trains: the tolerance is relative to the largest reference logit (>= 1)
        tol = PARANOID_TOLERANCE * max(1.0, float(ref.abs().max()))
        self._paranoid_checks = getattr(self, "_paranoid_checks", 0) + 1
        if not (err <= tol):
            raise ParanoidMismatch(f"vlsa_amd (VLSA_AMD_PARANOID): {what}: batched logits differ from the per-bag route by {err:.3e} "
                                   f"(> {tol:g}) for a bag of {tuple(X.shape)}; set VLSA_AMD_NO_DEFER=1 / "
                                   "VLSA_AMD_NO_LOOKAHEAD=1 to run without the shortcut and report this")
        return err

    # -- look-ahead: the reference handler's bag-by-bag evaluation loop at batched speed ---------------------------------------
    def _lookahead_hit(self, la, i, X, text_features=None):
        """the row of item i if la's windows hold it and the model state they were computed under still holds, else None.  The order
        -- row present, then text features, then state -- is what makes a hit cheap."""
        row = la["rows"].get(i)
        if row is None:
            return None
        if text_features is None:
            text_features = self._text_features()
        if not self._same_state(la["state"], self._eval_state(text_features)):
            return None
        la["used"] += 1
        la["last"] = i
        if i >= la["trigger"]:
            self._lookahead_extend(la, text_features)
        return self._lookahead_row(row, X)

    def _lookahead(self, src, X, text_features):
        """``net(X)`` in eval mode under ``no_grad`` for item i of a ``ResidentBags`` dataset (the handler's ``test_model`` loop,
        runner/vlsa_handler.py:322-330, calls the model once per bag): the first call of a window runs ``forward_bags`` over items
        i, i+1, ... (as many as are resident, <= ``lookahead_bags``: the loaders of base_handler.py:246-259 do not shuffle) -- ONE
        persistent launch instead of one latency-bound launch chain per bag -- and the following calls return their rows of that
        result; the first hit inside the newest window launches the window behind it, so the GPU is always one window ahead of
        the host walking through the rows (until round 4 the next window went out at the half-way hit: the GPU idled for half a
        window's host time per window).  Windows of slide-sized bags grow to 256 bags (``_lookahead_cap``).  A row is only ever handed out for the exact item it was computed from (the tag travels on the tensor object:
        ``ResidentBagView``) and while the model state it was computed under (``_eval_state``) still holds; any differentiable
        forward, ``_apply`` or ``load_state_dict`` drops the windows.  An access pattern that does not use its windows shrinks
        them (random access degenerates to the per-bag route)."""
        rb, i = src
        la = self._la
        same_rb = la is not None and la["rb"] is rb
        if same_rb and la["rows"]:
            hit = self._lookahead_hit(la, i, X, text_features)
            if hit is not None:
                return hit
        width, seq = int(self.lookahead_bags), 0
        if same_rb:
            width, seq = la["width"], la["seq"]
            if la["rows"]:                            # a miss behind a window: was that window used?
                if la["used"] >= la["computed"]:
                    width = min(self._lookahead_cap(la.get("mean_rows", 0)), 2 * width)
                elif la["used"] <= 1:
                    width = max(1, width // 4)
            seq = seq + 1 if i == la["last"] + 1 else 0
            if width <= 1 and seq >= 3:               # the per-bag route, but the accesses have become sequential again
                width = min(int(self.lookahead_bags), 8)
        self._la = la = {"rb": rb, "state": None, "rows": {}, "used": 0, "computed": 0, "width": width, "seq": seq, "last": i,
                         "hi": i - 1, "trigger": 1 << 62}
        if width <= 1:
            return None
        first = rb.resident_view(i)
        Xp = X.as_subclass(torch.Tensor)
        if first is None or first.data_ptr() != Xp.data_ptr() or tuple(first.shape) != tuple(Xp.shape[-2:]):
            return None                               # not (yet) the resident rows: the per-bag route
        la["state"] = self._eval_state(text_features, exact=True)      # the encoder is walked exactly before a window is computed
        if self._lookahead_window(la, text_features, width) < 2 and not la["rows"]:
            return None
        la["used"] = 1
        return self._lookahead_row(la["rows"][i], X) if i in la["rows"] else None

    def _lookahead_cap(self, mean_rows) -> int:
        """bags a window may hold: ``lookahead_bags``, more for slide-sized bags (<= 256, <= ``lookahead_rows`` rows per window)"""
        base = int(self.lookahead_bags)
        if mean_rows <= 0 or base <= 1:
            return base
        return max(base, min(VF.forward_max_bags(), int(self.lookahead_rows // max(1, int(mean_rows)))))

    def _lookahead_window(self, la, text_features, width) -> int:
        """run ``forward_bags`` over the resident items hi+1 .. hi+width of la's dataset and add their rows; -> number of bags"""
        rb, lo = la["rb"], la["hi"] + 1
        views = []
        for j in range(lo, min(len(rb), lo + width)):
            v = rb.resident_view(j)
            if v is None:
                break
            views.append(v)
        if not views or (len(views) < 2 and not la["rows"]):
            return len(views)                         # nothing to batch
        # the same windows come back every epoch: their checked bag set (descriptor rows, bags in flight) is kept on the dataset
        sets = rb.__dict__.setdefault("_la_sets", {})
        bagset = sets.get((lo, len(views)))
        if bagset is None or any(a is not b for a, b in zip(bagset, views)):
            if len(sets) > 256:
                sets.clear()
            bagset = sets[(lo, len(views))] = VF.BagSet(views)
        with torch.no_grad():
            out = self._forward_bags_fused(bagset, text_features)
        logits, feats, That = out[0], out[1], out[2]
        if ENV_PARANOID:
            j = random.randrange(len(views))
            self._paranoid_check(views[j], logits[j], f"look-ahead window of {len(views)} bags from item {lo}, bag {j}")
        per_bag = isinstance(feats, torch.Tensor) and feats.dim() == 2 and feats.shape[0] == len(views)
        # the rows are produced on the stream that is current NOW; a later hit may run under another current stream: an event per
        # window, waited for (on the consumer's stream) until the host has seen it complete
        win = {"ev": torch.cuda.Event(), "done": False}
        win["ev"].record()
        rows = la["rows"]
        for b in range(len(views)):
            rows[lo + b] = (logits[b:b + 1], feats[b:b + 1] if per_bag else None, That, per_bag, win)
        la["hi"] = lo + len(views) - 1
        la["computed"] += len(views)
        la["mean_rows"] = sum(v.shape[0] for v in views) / len(views)
        la["trigger"] = lo                            # the first hit in THIS window launches the one behind it (one window ahead)
        return len(views)

    def _lookahead_extend(self, la, text_features):
        """the newest window has been reached in order: launch the next one now -- the GPU is then always one window ahead of the
        host -- and forget the rows behind us"""
        la["trigger"] = 1 << 62
        if la["hi"] + 1 >= len(la["rb"]):
            return
        last = la["last"]
        for j in [j for j in la["rows"] if j < last]:
            del la["rows"][j]
        state = self._eval_state(text_features, exact=True)
        if not self._same_state(la["state"], state):
            return
        la["state"] = state
        la["width"] = min(self._lookahead_cap(la.get("mean_rows", 0)), 2 * max(la["width"], 1))     # used in order: the next window may be wider
        self._lookahead_window(la, text_features, la["width"])

    def _lookahead_row(self, row, X):
        logits, f, That, has_feats, win = row
        if not win["done"]:
            if win["ev"].query():
                win["done"] = True
            else:
                torch.cuda.current_stream(logits.device).wait_event(win["ev"])
        if not has_feats:       # identity FeatMIL: the per-patch unit features of THIS bag, as the per-bag route returns them
            f = VF.normalize_many(VF._bag2d(X.as_subclass(torch.Tensor))) if getattr(self, "return_patch_features", True) else None
        return logits, f, That

    def forward_bags(self, bags, ret_with_attn=False):
        """A list of independent bags in one call (the reference loops bag by bag: eval runner/vlsa_handler.py:315-345,
        training 260-289).  bf16 or fp32 bags with D == 512 and a VLFAN encoder go through the persistent multi-bag
        kernels, up to 64 bags per launch: fully fused when no gradient is needed, HIP aggregation forward + backward with
        a batched torch tail otherwise; anything else falls back to per-bag ``forward``.
        Returns (logits [B, K], image_features [B, D], text_features [K, D]); with ``ret_with_attn`` (VLFAN encoders) a
        fourth element: the per-bag attention weights ``[A_i [1, P, N_i]]`` of model/deepmil.py:198,206-215 -- from the same
        launch (the streaming kernel stores its scores, one more launch normalises them)."""
        enc = self.mil_encoder
        text_features = self._text_features()
        if ret_with_attn:
            return self._forward_bags_attn(bags, text_features)
        if self._needs_grad(text_features):
            self._invalidate(_FORWARD)           # a differentiable forward: parameters are about to move (see _lookahead)
            # (this site's own, looser condition, not ``uniform_bags``: the route behind it converts other dtypes through _bag2d)
            if (isinstance(enc, VLFAN) and len(bags) > 0
                    and all(x.is_cuda and x.dtype == bags[0].dtype and x.shape[-1] == 512 and x.shape[-2] > 0 for x in bags)):
                spec = enc.fused_head_spec()
                if (spec is not None and spec[0] == "mean" and text_features.is_cuda and text_features.shape[0] <= 64
                        and text_features.shape[1] == 512):
                    rows = enc.aggregate_bags(bags)          # [B, P, 512]: HIP forward + backward of the aggregation
                    if rows is not None:
                        # mean pooling + Linear / identity adapter + normalisation + cosine logits: two launches each way
                        return VF.head_train(rows, spec[2], spec[3], text_features, self.logit_scale, self._head_tickets)
                text_n = F.normalize(text_features, dim=-1)
                image_features = F.normalize(enc.forward_bags(bags), dim=-1)
                return self.logit_scale.exp() * image_features @ text_n.t(), image_features, text_n
            if isinstance(enc, mil_encoders.DeepMIL) and len(bags) > 0:
                return self._deepmil_logits(enc.forward_bags(bags), text_features)
            if isinstance(enc, FeatMIL) and enc.pooling not in ("mean", "max") and len(bags) > 0:
                routed = self._forward_bags_zeroshot_train(bags, text_features)
                if routed is not None:
                    return routed
            outs = [self.forward(x if x.dim() == 3 else x[None]) for x in bags]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), outs[0][2]
        with torch.no_grad():
            return self._forward_bags_fused(bags, text_features)

    def _forward_bags_zeroshot_train(self, bags, text_features):
        """Identity FeatMIL + logit pooling with a gradient to the text side (the prompt pre-training stage: trainable CoOp prompts
        and / or logit scale, cfg_zero_shot_conch.yaml): per chunk of 64 bags the launches of ``_forward_bags_zeroshot`` as ONE
        autograd node whose backward is one launch (``VF.zeroshot_pool_bags``).  Returns (logits [B, K], patch features as
        ``_forward_bags_zeroshot`` hands them out, T^ [K, 512] with the graph to the prompts); None: not this route's case (bags of
        several dtypes / another width / with a gradient of their own, more than 64 classes) -- the bag-by-bag calls serve it."""
        from .deepmil import _parse_logit_pooling
        T, ls = text_features, self.logit_scale
        if not (T.is_cuda and T.dim() == 2 and 1 <= T.shape[0] <= 64 and T.shape[1] == 512 and ls.is_cuda):
            return None
        bagset = bags if isinstance(bags, VF.BagSet) and bags.D == 512 else None
        flat = bagset if bagset is not None else [VF._bag2d(x) for x in bags]
        if not VF.uniform_bags(flat) or (bagset is None and any(x.requires_grad for x in flat)):
            return None
        k = _parse_logit_pooling(self.image_encoder_cfg["pooling"])
        if k is not None and not (1 <= k <= 32):
            return None
        outs = [VF.zeroshot_pool_bags(chunk, T, ls, k, return_text=True) for chunk in VF.bag_chunks(flat)]
        logits = VF.cat([o[0] for o in outs])
        feats = [VF.normalize_many(x) for x in flat] if getattr(self, "return_patch_features", None) is True else None
        return logits, feats, outs[0][1]

    def _train_head_takes(self, feats, T):
        """whether bag vectors [B, C] and text features T go through the one-node training head (``VF.head_train`` with P = 1)"""
        return (feats.is_cuda and feats.dtype == torch.float32 and feats.shape[1] % 4 == 0 and feats.shape[1] <= 1024 and T.is_cuda
                and T.dim() == 2 and 1 <= T.shape[0] <= 64 and T.shape[1] == feats.shape[1] and self.logit_scale.is_cuda)

    def _deepmil_logits(self, feats, text_features):
        """cosine logits of a DeepMIL batch's bag vectors [B, C], as the per-bag ``forward`` forms them: both normalisations and the
        logits as ONE autograd node (the batched training head with P = 1) where it applies, torch ops otherwise"""
        if self._train_head_takes(feats, text_features):
            return VF.head_train(feats.unsqueeze(1).contiguous(), None, None, text_features, self.logit_scale, self._head_tickets)
        text_n = F.normalize(text_features, dim=-1)
        image_features = F.normalize(feats.float(), dim=-1)
        return self.logit_scale.exp() * image_features @ text_n.t(), image_features, text_n

    def _forward_bags_attn(self, bags, text_features):
        enc = self.mil_encoder
        if isinstance(enc, mil_encoders.DeepMIL):
            # (gated-)attention pooling: the batched route hands back the per-bag attention of forward(x, ret_with_attn=True)
            with torch.set_grad_enabled(self._needs_grad(text_features)):
                feats, attn = enc.forward_bags(bags, ret_with_attn=True)
                return (*self._deepmil_logits(feats, text_features), attn)
        if not isinstance(enc, VLFAN):
            raise NotImplementedError("ret_with_attn over a list of bags is the VLFAN / DeepMIL encoders' output (model/deepmil.py:206-215)")
        grad = self._needs_grad(text_features)
        spec = enc.fused_head_spec()
        flat = [VF._bag2d(x) for x in bags]
        if grad or spec is None or spec[0] == "module" or not VF.uniform_bags(flat):
            with torch.set_grad_enabled(grad):
                text_n = F.normalize(text_features, dim=-1)
                feats, attn = enc.forward_bags(bags, ret_with_attn=True)
                feats = F.normalize(feats, dim=-1)
                return self.logit_scale.exp() * feats @ text_n.t(), feats, text_n, attn
        with torch.no_grad():
            logits, feats, That, plans = self._forward_bags_fused(flat, text_features, want_attn=True)
        attn = [a.unsqueeze(0).clone() for pl in plans for a in pl.attn.views]   # the plan's buffers are reused by later calls
        return logits, feats, That, attn

    def _forward_bags_fused(self, bags, text_features, want_attn=False, trusted=False):
        """trusted: the bags are [N, 512] device views of ONE dtype with N > 0 (the resident arena's own views): per-bag checks are
        skipped -- with 64 small bags per call they are most of the host time"""
        enc = self.mil_encoder
        spec = enc.fused_head_spec() if isinstance(enc, VLFAN) else None
        bagset = bags if isinstance(bags, VF.BagSet) else None      # checked once (vlsa_amd.functional.BagSet): trusted, rows kept
        trusted = trusted or bagset is not None
        flat = bags if bagset is not None else (list(bags) if trusted else [VF._bag2d(x) for x in bags])
        projected = False
        if (getattr(enc, "feat_proj", None) is not None and isinstance(enc, (VLFAN, mil_encoders.DeepMIL)) and len(flat) > 0
                and all(x.is_cuda and x.shape[0] > 0 for x in flat)):
            flat = enc.feat_proj.forward_bags(flat)    # use_feat_proj=True: one fused HIP launch per 64 bags, fp32 [N, 512] out
            projected = True
        ok = (spec is not None and spec[0] != "module" and len(flat) > 0
              and ((trusted and not projected) or VF.uniform_bags(flat)))
        if not ok:
            same = VF.uniform_bags(flat)
            if same and isinstance(enc, FeatMIL) and enc.pooling not in ("mean", "max") and text_features.shape[0] <= 64:
                return self._forward_bags_zeroshot(flat, text_features)
            if same and isinstance(enc, FeatMIL) and enc.pooling in ("mean", "max"):
                # FeatMIL baseline (model/deepmil.py:57-60): row means / column maxima of all bags in two launches per 64 bags
                # (one bag per call: the single-bag launch pair; torch.cat over one chunk too, as the route recording pins), then normalise + logits
                f = mil_encoders.pool_mean_max(flat, enc.pooling, join=torch.cat)
                That = F.normalize(text_features.detach().float(), dim=-1)
                feats = F.normalize(f, dim=-1)
                return self.logit_scale.exp() * feats @ That.t(), feats, That
            if same and isinstance(enc, mil_encoders.DeepMIL) and (enc.feat_proj is None or projected):
                return self._forward_bags_deepmil(flat, text_features)
            if isinstance(enc, VLFAN) and (enc.feat_proj is None or projected) and same:
                # pooling over the queries by a module (attention / gated attention): batched HIP aggregation, then the
                # module, the adapter and the cosine logits as batched torch ops on [B, P, 512]
                That = F.normalize(text_features, dim=-1)
                feats = F.normalize(enc.forward_bags(flat, projected=projected), dim=-1)
                return self.logit_scale.exp() * feats @ That.t(), feats, That
            outs = [self.forward(x if x.dim() == 3 else x[None]) for x in bags]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), outs[0][2]
        mode, pw, W, b = spec
        Qsrc = enc.step_query()
        Q, T, ls, Wc, bc, pwc = self._f32_operands(Qsrc, text_features, W, b, pw)
        pkey = self._params_key(enc, Qsrc, text_features) if isinstance(Qsrc, torch.Tensor) else None
        P = Q.shape[0] - (1 if enc.gated_query else 0)
        K = text_features.shape[0]
        logits, feats, That, used = [], [], None, []
        # bags per persistent launch: 64 x 50k-patch bags are 3.3 GB per launch already; slide-sized bags (the reference's TCGA bags:
        # 2-12k patches) go up to the forward kernels' 256 per launch -- the launch's fixed latency chain and the host calls are
        # paid per launch (2 798-patch bags: 0.62 -> 0.47 us per bag in the streaming kernel)
        step = 64
        if len(flat) > 64:
            rows = sum(bagset.sizes if bagset is not None else [x.shape[0] for x in flat]) / len(flat)
            while step < VF.forward_max_bags() and step < len(flat) and 2 * step * rows <= 64 * 50_000:
                step *= 2
        # several launches: they alternate between two side streams (a plan per parity: its own workspace and outputs), so that the
        # merge / head launches of chunk i run under the streaming kernel of chunk i + 1 -- the tail kernels fit next to a persistent
        # workgroup (<= 96 VGPRs, <= 8 KiB LDS) -- the way bench.py issues its launches
        n_chunks = (len(flat) + step - 1) // step
        side = None
        if n_chunks > 1 and not want_attn:
            dev0 = flat[0].device
            side = self.__dict__.get("_side_streams")
            if side is None or side[0].device != dev0:
                side = self.__dict__["_side_streams"] = (torch.cuda.Stream(device=dev0), torch.cuda.Stream(device=dev0))
            cur = torch.cuda.current_stream(dev0)
            for st_ in side:
                st_.wait_stream(cur)
        for ci, i in enumerate(range(0, len(flat), step)):
            chunk = bagset.chunk(i, step) if (bagset is not None and not projected) else flat[i:i + step]
            key = ("batch", len(chunk), P, K, chunk[0].device, enc.gated_query, mode, W is None, want_attn, i if want_attn else (ci & 1))
            plan = self._plans.get(key)
            if plan is None:
                plan = VF.VlfanBatchPlan(len(chunk), P, K, chunk[0].device, gated=enc.gated_query, pool=mode,
                                         identity_head=W is None, coattn_scale=float(enc.coattn_logit_scale.exp()),
                                         reserved_cus=0, want_attn=want_attn)
                self._plans[key] = plan
            used.append(plan)
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=chunk[0].device)  # noqa: E731
            outs = {"logits": f(len(chunk), K), "vhat": f(len(chunk), 512)}
            if That is None:
                outs["That"] = That = f(K, 512)
            if side is not None:
                with torch.cuda.stream(side[ci & 1]):
                    plan.set_bags(chunk, validated=True)
                    plan.run(Q, T, ls, Wc, bc, pwc, outs=outs, params_key=pkey)
            else:
                plan.set_bags(chunk, validated=True)
                plan.run(Q, T, ls, Wc, bc, pwc, outs=outs, params_key=pkey)
            logits.append(outs["logits"])
            feats.append(outs["vhat"])
        if side is not None:
            for st_ in side:
                cur.wait_stream(st_)
        res = (logits[0], feats[0], That) if len(logits) == 1 else (torch.cat(logits), torch.cat(feats), That)
        return res + (used,) if want_attn else res

    def _forward_bags_zeroshot(self, flat, text_features):
        """Identity FeatMIL + logit pooling for a list of bags (the reference's eval loop is encoder-agnostic,
        runner/vlsa_handler.py:315-345): per chunk of 64 bags one persistent streaming launch that stores the per-class
        cosines and one launch that pools them -- instead of ~8 launches per bag.  The unit-norm patch features the reference
        hands back per bag ([N_i, D] fp32 each) are only produced when ``return_patch_features`` is set to True explicitly."""
        from .deepmil import _parse_logit_pooling
        k = _parse_logit_pooling(self.image_encoder_cfg["pooling"])
        T = text_features.detach().float().contiguous()
        logits = torch.cat([VF.zeroshot_pool_bags(chunk, T, self.logit_scale.detach(), k) for chunk in VF.bag_chunks(flat)])
        That, _ = VF.normalize_rows(T)
        feats = [VF.normalize_many(x) for x in flat] if getattr(self, "return_patch_features", None) is True else None
        return logits, feats, That

    def _forward_bags_deepmil(self, flat, text_features):
        """DeepMIL encoder over a list of bags: the N-sized part (attention scores + softmax-weighted row sum) in one score
        launch and one pooling launch per <= 64 bags (``DeepMIL.pool_bags``), then ONE batched tail for all bags (head,
        normalise, cosine logits on [B, 512])."""
        enc = self.mil_encoder
        v = enc.head(enc.pool_bags(flat))                                            # [B, 512]
        That = F.normalize(text_features.detach().float(), dim=-1)
        feats = F.normalize(v, dim=-1)
        return self.logit_scale.exp() * feats @ That.t(), feats, That

    def _forward_zeroshot(self, X, text_features):
        """Identity FeatMIL: per-patch cosine logits pooled over the patches (model/vlsa.py:194-196)."""
        from .deepmil import _parse_logit_pooling
        assert X.shape[0] == 1
        X2 = VF._bag2d(X)
        N = X2.shape[0]
        topk = _parse_logit_pooling(self.image_encoder_cfg["pooling"])
        cosines = VF.class_cosines(X2, text_features.detach())                 # [K, N]
        pooled = VF.topk_mean(cosines, N if topk is None else min(topk, N))      # [K]
        logits = (self.logit_scale.exp() * pooled)[None, :]
        That, _ = VF.normalize_rows(text_features.detach())
        # the reference hands back the unit-norm patch features [N, D] here (identity encoder); 4 * N * D bytes per call that
        # its handler never reads -- ``return_patch_features = False`` skips them (None is returned in their place)
        image_features = VF.normalize_many(X2) if getattr(self, "return_patch_features", True) else None
        return logits, image_features, That

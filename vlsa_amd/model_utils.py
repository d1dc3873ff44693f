"""Model factory with the reference's names and signatures (model/utils.py:13-45, model/prompt_encoder.py:22-33,
model/prompt_learners/__init__.py:6-24): what ``VLSAHandler.func_load_model`` reaches through
``load_model(cfg['arch'], **arch_cfg)`` (runner/vlsa_handler.py:112-120).

    load_model('VLSA', text_encoder_cfg=..., image_encoder_cfg=..., prompt_learner_cfg=..., pretrained_prompt_learner_cfg=...,
               vlsa_api=..., path_clip_model=...)  ->  vlsa_amd.vlsa.VLSA
    load_model('DeepMIL', [512, 256, 4], network='ABMIL' | 'MaxMIL' | 'MeanMIL' | 'DSMIL', ...)  ->  vlsa_amd.deepmil.DeepMIL / DSMIL
               (what ``SAHandler.func_load_model`` reaches, runner/sa_handler.py)

``patch_reference()`` is the one-line swap for a process running the reference's code: it points the reference's factory
(and its MIL-encoder name lookup) at the classes of this package, after which ``runner/vlsa_handler.py`` runs unmodified --
construction, freezing (126-149), ``.cuda()``, the per-bag training / evaluation loops (260-345) and checkpoint loading.
"""
from __future__ import annotations

from typing import List, Optional

__all__ = ["load_model", "Deep_VLSA", "get_prompt_encoder", "load_prompt_learner", "load_prompt_adapter", "patch_reference",
           "patch_reference_deepattnmisl", "unpatch_reference_deepattnmisl", "patch_reference_ilra", "unpatch_reference_ilra", "arch_cfg_from_run_cfg", "func_load_model"]


_MISSING_DEPENDENCY = {"TransMIL": "nystrom_attention (NystromAttention)", "ILRA": "nystrom_attention (via model/deepmil.py's imports)",
                       "DeepAttnMISL": "the per-slide cluster labels of its dataset pipeline", "PatchGCN": "torch_geometric"}


def load_model(arch: str, dims: Optional[List] = None, **kws):
    """model/utils.py:13-36.  ``'VLSA'`` builds the language-guided model; ``'DeepMIL'`` builds the survival baselines of
    ``runner/sa_handler.py`` that have HIP kernels here -- ``network='ABMIL' | 'MaxMIL' | 'MeanMIL'`` (``vlsa_amd.deepmil.DeepMIL``,
    with the reference's ``pooling`` assertions) and ``'DSMIL'`` (``vlsa_amd.deepmil.DSMIL``) -- from ``dims = [dim_in, dim_hid,
    num_cls]``.  DSMIL's backward reaches its own eight parameters, not the bag rows: with ``use_feat_proj=True`` (the constructor's
    default; every shipped cfg_sa_base_conch.yaml sets False) freeze ``model.feat_proj`` before training, or the first step raises.
    TransMIL / PatchGCN are not served, and DeepAttnMISL / ILRA not THROUGH THIS FACTORY: NotImplementedError names what they would need.
    ILRA is served as ``vlsa_amd.deepmil.ILRA`` (``forward(X)``, ``forward_bags(bags)``: softmax pooling and the row map in HIP, forward
    and backward); build it directly, or call ``patch_reference_ilra()`` and let the reference's own factory build it.
    DeepAttnMISL itself is served as ``vlsa_amd.deepmil.DeepAttnMISL`` (``forward(X, cluster_id)``, ``forward_bags(bags, cluster_ids)``:
    phi + per-cluster mean in HIP); build it directly, or call ``patch_reference_deepattnmisl()`` and let the reference's own factory
    and handler (which hands the model the cluster ids of its dataset pipeline) build and drive it."""
    if arch == "VLSA":
        return Deep_VLSA(**kws)
    if arch == "DeepMIL":
        assert "network" in kws, "Please specify a network for a DeepMIL arch."
        network = kws["network"]
        from .deepmil import DSMIL, DeepMIL
        if network == "ABMIL":                      # model/utils.py:72-77
            if "pooling" in kws:
                assert kws["pooling"] in ["attention", "gated_attention"]
            return DeepMIL(dims[0], dims[1], dims[2], **kws)
        if network in ("MaxMIL", "MeanMIL"):        # model/utils.py:79-91
            pooling = "max" if network == "MaxMIL" else "mean"
            if "pooling" in kws:
                assert kws["pooling"] == pooling
            return DeepMIL(dims[0], dims[1], dims[2], **dict(kws, pooling=pooling))
        if network == "DSMIL":                      # model/utils.py:67-70
            return DSMIL(dims[0], dims[1], dims[2], **kws)
        if network in _MISSING_DEPENDENCY:
            raise NotImplementedError(f"network={network!r} has no HIP implementation in this package (the reference's needs "
                                      f"{_MISSING_DEPENDENCY[network]}); use the reference's own factory for it")
        raise NotImplementedError(f"DeepMIL network {network!r} cannot be recognized")
    raise NotImplementedError("Backbone {} cannot be recognized".format(arch))


def Deep_VLSA(**kws):
    """model/utils.py:40-45"""
    for need in ("text_encoder_cfg", "image_encoder_cfg", "prompt_learner_cfg"):
        assert need in kws
    from .vlsa import VLSA
    return VLSA(**kws)


def get_prompt_encoder(vl_model, api):
    """model/prompt_encoder.py:22-33.  CONCH: the HIP text tower adopting ``vl_model.text``; CLIP / HF: the same tower machinery over
    the text side of an OpenAI CLIP model / a ``transformers`` ``CLIPModel`` (QuickGELU, <eot> pooling)."""
    from . import prompt_encoder as pe
    classes = {"CONCH": pe.CONCHPromptEncoder, "CLIP": pe.CLIPPromptEncoder, "HF": pe.HFCLIPPromptEncoder}
    if api in classes:
        return classes[api](vl_model)
    raise ValueError(f"Got an invalid api ({api}).")


def load_prompt_learner(learner_name: str, cfg: dict):
    """model/prompt_learners/__init__.py:6-18: 'plain' | 'rank'; anything else yields None there too."""
    from .prompt_learner import PlainPromptLearner, RankPromptLearner
    if learner_name == "plain":
        return PlainPromptLearner(**cfg)
    if learner_name == "rank":
        return RankPromptLearner(**cfg)
    return None


def load_prompt_adapter(prompt_encoder, cfg: dict):
    """model/prompt_learners/__init__.py:20-24"""
    from .prompt_adapter import PromptAdapter
    return PromptAdapter(prompt_encoder, **cfg)


_ABSENT = object()      # patch_reference: the patched module did not have the attribute


def _sub_cfg(cfg: dict, prefix: str) -> dict:
    """the keys ``<prefix>_<name>`` of a flat run config as ``{name: value}`` (what utils/func.py:136-147 ``fetch_kws`` hands the
    handler; names shorter than two characters are not picked up there either)"""
    cut = len(prefix) + 1
    return {k[cut:]: v for k, v in cfg.items() if k.startswith(prefix) and len(k) > cut and k[len(prefix)] == "_"}


def arch_cfg_from_run_cfg(cfg: dict) -> dict:
    """A run's flat config (cfg_vlsa_conch.yaml / a run directory's config.yaml) -> the keyword arguments of
    ``load_model('VLSA', **arch_cfg)``, as ``VLSAHandler.func_load_model`` assembles them (runner/vlsa_handler.py:88-120)."""
    arch = cfg["arch"].lower()
    assert f"{arch}_api" in cfg, "Please specify the API for VLSA models."
    learner = cfg["vlsa_pmt_learner_name"]
    learner_cfg = _sub_cfg(cfg, f"{arch}_pmt_learner_{learner.lower()}")
    pretrained = bool(cfg.get("vlsa_pmt_learner_pretrained", False))
    learner_cfg.update(name=learner, pretrained=pretrained)
    coop_cfg = None
    if pretrained:          # text prompts pre-trained by CoOp: the checkpoint path is a template over (split seed, method)
        coop_cfg = _sub_cfg(cfg, "vlsa_pmt_learner_coop")
        assert coop_cfg.get("ckpt") is not None, "Found null ckpt path."
        coop_cfg["ckpt"] = coop_cfg["ckpt"].format(cfg["data_split_seed"], coop_cfg["method"])
    return dict(vlsa_api=cfg[f"{arch}_api"], text_encoder_cfg=_sub_cfg(cfg, f"{arch}_txt_encoder"),
                image_encoder_cfg=_sub_cfg(cfg, f"{arch}_img_encoder"), prompt_learner_cfg=learner_cfg,
                pretrained_prompt_learner_cfg=coop_cfg, path_clip_model=cfg["path_clip_model"])


def func_load_model(cfg: dict):
    """``VLSAHandler.func_load_model`` (runner/vlsa_handler.py:88-151) without the handler: build the model from a run config and
    freeze what the config freezes (prompt embeddings, MIL encoder, text tower, logit scale).  ``init_wt`` (a generic re-init of
    every Linear, off in every shipped config) is refused rather than silently ignored."""
    if cfg.get("init_wt"):
        raise NotImplementedError("init_wt: True re-initialises the model with utils/func.py:general_init_weight; run it on the result if wanted")
    arch_cfg = arch_cfg_from_run_cfg(cfg)
    model = load_model(cfg["arch"], **arch_cfg)
    arch = cfg["arch"].lower()
    learner = cfg["vlsa_pmt_learner_name"]
    freeze = []
    if learner == "CoOp":
        freeze += [(model.prompt_learner.context_embeds, arch_cfg["prompt_learner_cfg"]["frozen_context_embeds"]),
                   (model.prompt_learner.rank_embeds, arch_cfg["prompt_learner_cfg"]["frozen_rank_embeds"])]
    if learner in ("CoOp", "Adapter"):
        tower = model.prompt_encoder if hasattr(model, "prompt_encoder") else getattr(model, "text_encoder", None)
        freeze += [(model.mil_encoder, arch_cfg["image_encoder_cfg"]["frozen"]), (tower, arch_cfg["text_encoder_cfg"]["frozen"]),
                   (model.logit_scale, cfg[f"{arch}_frozen_logit_scale"])]
    for obj, frozen in freeze:
        if frozen and obj is not None:
            for p in (obj.parameters() if hasattr(obj, "parameters") else [obj]):
                p.requires_grad = False
    return model


def patch_reference(resident_bags: bool = False, defer_training_calls: bool = True, **resident_kw):
    """Point the reference's factory at this package (call once, before the handler is built):

        import vlsa_amd.model_utils; vlsa_amd.model_utils.patch_reference()

    * ``model.utils.VLSA`` -> ``vlsa_amd.vlsa.VLSA``: ``load_model('VLSA', **arch_cfg)`` (model/utils.py:36,44) then builds the HIP
      model from the handler's unmodified ``arch_cfg``;
    * ``model.deepmil.{VLFAN, FeatMIL, DeepMIL, logit_pooling}`` -> this package's: the name lookup of
      model/utils_vl.py:129-138 and ``utils/model_inference.py`` see the same classes.
    * ``model.prompt_encoder.{CLIPPromptEncoder, HFCLIPPromptEncoder}`` -> this package's, when that module is importable: the
      reference's own ``get_prompt_encoder(vl_model, 'CLIP' | 'HF')`` (model/prompt_encoder.py:22-33) then builds the HIP towers.
    * ``model.utils.DeepMIL``, ``model.utils.DSMIL`` and ``model.deepmil.DSMIL`` -> this package's: ``load_model('DeepMIL', dims,
      network='ABMIL' | 'MaxMIL' | 'MeanMIL' | 'DSMIL')`` (model/utils.py:67-91), i.e. ``SAHandler.func_load_model``, builds the
      HIP baselines.
    * ``resident_bags=True``: ``dataset.utils.prepare_surv_dataset`` (and the name ``runner.sa_handler`` imported from it, if already
      loaded) wraps what it returns in ``vlsa_amd.ingest.ResidentBags`` -- every bag is read and uploaded ONCE, later epochs find it in
      HBM.  Stored as **fp32** here, bit for bit what dataset/PatchWSI.py:214 hands the handler (an "unmodified" reference run must
      not be fed rounded features silently); ``dtype=torch.bfloat16`` in ``resident_kw`` halves the footprint and the streaming
      time at ~1e-2 on the logits.  Needs ``num_workers: 0`` in the run's config (a worker process has no device: items pass
      through unchanged there, with a one-time warning).
    * ``defer_training_calls`` (default True): ``VLSA.defer_training_calls`` -- the handler's ``net(xs[i])`` calls of a training batch run
      as ONE batched forward the moment ``torch.cat(y_hat)`` looks at them (vlsa_amd/deferred.py): 1.9 instead of 4.5 ms per 32-bag step.
    Returns the patched reference modules (for un-patching in tests)."""
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    import model.vlsa as ref_vlsa
    from . import deepmil as fast
    from .vlsa import VLSA
    saved = dict(VLSA_utils=ref_utils.VLSA, VLSA_vlsa=ref_vlsa.VLSA, VLFAN=ref_mil.VLFAN, FeatMIL=ref_mil.FeatMIL,
                 DeepMIL=ref_mil.DeepMIL, logit_pooling=ref_mil.logit_pooling)
    ref_utils.VLSA = VLSA
    ref_vlsa.VLSA = VLSA
    # the handler's bag-by-bag training loop (runner/vlsa_handler.py:260-289) at the batched step's speed: its net(X) calls are recorded
    # and run as ONE forward_bags when torch.cat first looks at a prediction (vlsa_amd/deferred.py)
    saved["defer_training_calls"] = VLSA.defer_training_calls
    VLSA.defer_training_calls = defer_training_calls
    ref_mil.VLFAN, ref_mil.FeatMIL, ref_mil.DeepMIL = fast.VLFAN, fast.FeatMIL, fast.DeepMIL
    ref_mil.logit_pooling = ref_vlsa.logit_pooling = fast.logit_pooling
    # the SA baselines' factory names (model/utils.py:6 imported them by name)
    saved["sa_baselines"] = [(mod, attr, getattr(mod, attr, _ABSENT)) for mod, attr in
                             ((ref_utils, "DeepMIL"), (ref_utils, "DSMIL"), (ref_mil, "DSMIL"))]
    ref_utils.DeepMIL, ref_utils.DSMIL, ref_mil.DSMIL = fast.DeepMIL, fast.DSMIL, fast.DSMIL
    try:                                   # (absent where only a part of the reference's tree is importable)
        import model.prompt_encoder as ref_pe
    except ImportError:
        ref_pe = None
    if ref_pe is not None:
        from . import prompt_encoder as pe
        saved["prompt_encoders"] = [(ref_pe, attr, getattr(ref_pe, attr, _ABSENT)) for attr in ("CLIPPromptEncoder", "HFCLIPPromptEncoder")]
        ref_pe.CLIPPromptEncoder, ref_pe.HFCLIPPromptEncoder = pe.CLIPPromptEncoder, pe.HFCLIPPromptEncoder
    if resident_bags:
        import sys
        import dataset.utils as ref_ds
        from .ingest import ResidentBags
        original = ref_ds.prepare_surv_dataset
        if not getattr(original, "_vlsa_resident", False):
            import torch
            resident_kw.setdefault("dtype", torch.float32)

            def prepare_surv_dataset(*args, **kwargs):
                return ResidentBags(original(*args, **kwargs), **resident_kw)
            prepare_surv_dataset._vlsa_resident = True
            prepare_surv_dataset.__wrapped__ = original
            saved["prepare_surv_dataset"] = original
            ref_ds.prepare_surv_dataset = prepare_surv_dataset
            for name in ("runner.sa_handler", "runner.vlsa_handler", "runner.base_handler"):
                mod = sys.modules.get(name)
                if mod is not None and getattr(mod, "prepare_surv_dataset", None) is original:
                    mod.prepare_surv_dataset = prepare_surv_dataset
    return saved


def patch_reference_deepattnmisl():
    """Point the reference's DeepAttnMISL at this package's (separate from ``patch_reference``, which stays as it is):
    ``model.deepmil.DeepAttnMISL`` and ``model.utils.DeepAttnMISL`` -- what ``load_model('DeepMIL', dims, network='DeepAttnMISL')``
    (model/utils.py) builds -- and, if ``runner.sa_handler`` is loaded, the name its ``isinstance`` checks read.  Returns what it
    replaced, for ``unpatch_reference_deepattnmisl``."""
    import sys
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    from .deepmil import DeepAttnMISL
    mods = [ref_mil, ref_utils]
    handler = sys.modules.get("runner.sa_handler")
    if handler is not None:
        mods.append(handler)
    saved = [(mod, getattr(mod, "DeepAttnMISL", _ABSENT)) for mod in mods]
    for mod in mods:
        mod.DeepAttnMISL = DeepAttnMISL
    return saved


def unpatch_reference_deepattnmisl(saved) -> None:
    """Undo ``patch_reference_deepattnmisl`` (``saved`` = what it returned)."""
    for mod, original in saved:
        if original is _ABSENT:
            if hasattr(mod, "DeepAttnMISL"):
                delattr(mod, "DeepAttnMISL")
        else:
            mod.DeepAttnMISL = original


def patch_reference_ilra():
    """Point the reference's ILRA at this package's (separate from ``patch_reference``, which stays as it is): ``model.deepmil.ILRA`` and
    ``model.utils.ILRA`` -- what ``load_model('DeepMIL', dims, network='ILRA')`` (model/utils.py) builds -- and, if ``runner.sa_handler``
    is loaded and carries the name, that one too.  Returns what it replaced, for ``unpatch_reference_ilra``."""
    import sys
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    from .deepmil import ILRA
    mods = [ref_mil, ref_utils]
    handler = sys.modules.get("runner.sa_handler")
    if handler is not None and hasattr(handler, "ILRA"):
        mods.append(handler)
    saved = [(mod, getattr(mod, "ILRA", _ABSENT)) for mod in mods]
    for mod in mods:
        mod.ILRA = ILRA
    return saved


def unpatch_reference_ilra(saved) -> None:
    """Undo ``patch_reference_ilra`` (``saved`` = what it returned)."""
    for mod, original in saved:
        if original is _ABSENT:
            if hasattr(mod, "ILRA"):
                delattr(mod, "ILRA")
        else:
            mod.ILRA = original


def unpatch_reference(saved) -> None:
    """Undo ``patch_reference`` (``saved`` = what it returned): the reference's own classes, dataset factory and the class-wide
    ``VLSA.defer_training_calls`` flag are back as they were."""
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    import model.vlsa as ref_vlsa
    from .vlsa import VLSA
    ref_utils.VLSA, ref_vlsa.VLSA = saved["VLSA_utils"], saved["VLSA_vlsa"]
    ref_mil.VLFAN, ref_mil.FeatMIL, ref_mil.DeepMIL = saved["VLFAN"], saved["FeatMIL"], saved["DeepMIL"]
    ref_mil.logit_pooling = ref_vlsa.logit_pooling = saved["logit_pooling"]
    for mod, attr, original in list(saved.get("sa_baselines", ())) + list(saved.get("prompt_encoders", ())):
        if original is _ABSENT:
            if hasattr(mod, attr):
                delattr(mod, attr)
        else:
            setattr(mod, attr, original)
    VLSA.defer_training_calls = saved.get("defer_training_calls", False)
    if "prepare_surv_dataset" in saved:
        import sys
        import dataset.utils as ref_ds
        patched = ref_ds.prepare_surv_dataset
        ref_ds.prepare_surv_dataset = saved["prepare_surv_dataset"]
        for name in ("runner.sa_handler", "runner.vlsa_handler", "runner.base_handler"):
            mod = sys.modules.get(name)
            if mod is not None and getattr(mod, "prepare_surv_dataset", None) is patched:
                mod.prepare_surv_dataset = saved["prepare_surv_dataset"]

"""Host-side hooks of the model factory: where the tokenizer and the pretrained VL model come from.

The reference builds both inside ``VLSA.__init__`` (model/vlsa.py:38-49: ``Tokenizer(root, name, api)`` from
model/utils_vl.py:19-75 and ``load_vl_model_to_cpu`` from model/utils_vl.py:78-149).  Tokenisation and weight download /
deserialisation are host glue outside the hot path, so this package does not re-implement them: it
calls a *hook*.

    set_tokenizer_factory(fn)    fn(root=..., name=..., api=...) -> tokenizer with the reference wrapper's contract:
                                 ``tok(text | [texts], return_raw_tokens, return_num_tokens)`` and the attributes
                                 ``bos_token_id / eos_token_id / pad_token_id``
    set_vl_model_loader(fn)      fn(text_encoder_cfg=..., root=..., api=...) -> object with ``.logit_scale`` and what the API's prompt
                                 encoder adopts (model/prompt_encoder.py): CONCH ``.text`` (a CoCa text tower, 213-243); CLIP
                                 ``.transformer / .positional_embedding / .ln_final / .text_projection / .token_embedding`` (39-47);
                                 HF ``.text_model`` and ``.text_projection`` of a ``transformers`` ``CLIPModel`` (106-127)

Defaults (no hook installed): the host application's own loaders when they are importable -- running inside the reference's
tree, ``model.utils_vl.Tokenizer`` and ``model.conch.create_model_from_pretrained`` (the calls model/utils_vl.py:27-41,116-123
make); otherwise the ``conch`` pip package of mahmoodlab/CONCH.  Neither being importable raises with instructions; nothing
here falls back to a CPU computation of the hot path.

The CLIP and HF defaults read LOCAL files only -- nothing here downloads (the reference's ``clip._download`` is not reached):

    CLIP   ``<root>/openai_clip/<name with '/' as '-'>.pt`` (where model/utils_vl.py:96-100 stores 'ViT-B/16' as ViT-B-16.pt): a
           TorchScript archive or a pickled state dict in OpenAI's layout; only its text side is built (``load_openai_clip_text``)
    HF     the directory ``<root>/<name>`` ('openai/clip-vit-base-patch16', 'vinid/plip') through
           ``transformers.CLIPModel.from_pretrained(..., local_files_only=True)``
A missing file raises ``FileNotFoundError`` with the path that was expected.
"""
from __future__ import annotations

import os.path as osp
from typing import Callable, Optional

_tokenizer_factory: Optional[Callable] = None
_vl_model_loader: Optional[Callable] = None


def set_tokenizer_factory(fn: Optional[Callable]) -> Optional[Callable]:
    """Install (or, with None, remove) the tokenizer hook; returns the previous one."""
    global _tokenizer_factory
    prev, _tokenizer_factory = _tokenizer_factory, fn
    return prev


def set_vl_model_loader(fn: Optional[Callable]) -> Optional[Callable]:
    """Install (or, with None, remove) the VL-model hook; returns the previous one."""
    global _vl_model_loader
    prev, _vl_model_loader = _vl_model_loader, fn
    return prev


def make_tokenizer(root, name, api):
    if _tokenizer_factory is not None:
        return _tokenizer_factory(root=root, name=name, api=api)
    try:
        from model.utils_vl import Tokenizer            # the host application's wrapper (reference tree on sys.path)
    except Exception as exc:
        raise RuntimeError("no tokenizer: call vlsa_amd.hooks.set_tokenizer_factory(fn) -- fn(root, name, api) must return an "
                           "object with the contract of the reference's model.utils_vl.Tokenizer -- or run inside the "
                           "reference's tree, where that class is importable") from exc
    return Tokenizer(root=root, name=name, api=api)


def load_vl_model(text_encoder_cfg, root, api):
    if _vl_model_loader is not None:
        return _vl_model_loader(text_encoder_cfg=text_encoder_cfg, root=root, api=api)
    if api == "CLIP":
        return load_openai_clip_text(osp.join(root, "openai_clip", text_encoder_cfg["name"].replace("/", "-") + ".pt"))
    if api == "HF":
        path = osp.join(root, text_encoder_cfg["name"])
        if not osp.isfile(osp.join(path, "config.json")):
            raise FileNotFoundError(f"vlsa_api='HF': no HuggingFace CLIP model directory (config.json + weights) at {path}")
        from transformers import CLIPModel
        return CLIPModel.from_pretrained(path, local_files_only=True)
    if api != "CONCH":
        raise ValueError(f"Got an invalid api ({api}).")
    ckpt = osp.join(root, text_encoder_cfg["name"], "pytorch_model.bin")
    create = None
    try:
        from model.conch import create_model_from_pretrained as create          # reference tree
    except Exception:
        try:
            from conch.open_clip_custom import create_model_from_pretrained as create   # mahmoodlab/CONCH package
        except Exception as exc:
            raise RuntimeError("no CONCH model loader: call vlsa_amd.hooks.set_vl_model_loader(fn), or make the reference's "
                               "`model.conch` / the `conch` package importable") from exc
    return create("conch_ViT-B-16", checkpoint_path=ckpt, return_transform=False)


def load_openai_clip_text(path):
    """The text side of an OpenAI CLIP checkpoint on the CPU: ``path`` is the ``.pt`` file OpenAI distributes (a TorchScript archive)
    or a pickled state dict in the same layout (model/clip/model.py:399-436 reads the same keys).  Sizes come from the tensors:
    width = ``ln_final.weight``, heads = width / 64, blocks counted from the keys.  fp16 tensors are widened to fp32 (exact)."""
    import torch
    import torch.nn as nn
    from .prompt_encoder import CLIPPromptEncoder
    if not osp.isfile(path):
        raise FileNotFoundError(f"vlsa_api='CLIP': no OpenAI CLIP checkpoint at {path} (this package reads local files only; "
                                "put the .pt file there, or install a loader with vlsa_amd.hooks.set_vl_model_loader)")
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location="cpu")
    if hasattr(sd, "state_dict"):          # a pickled module
        sd = sd.state_dict()
    sd = {k: v.float() for k, v in sd.items()
          if k.split(".")[0] in ("transformer", "positional_embedding", "ln_final", "text_projection", "token_embedding", "logit_scale")}
    width = sd["ln_final.weight"].shape[0]
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    tower = CLIPPromptEncoder(width=width, heads=width // 64, layers=layers, context_length=sd["positional_embedding"].shape[0],
                              vocab_size=sd["token_embedding.weight"].shape[0], output_dim=sd["text_projection"].shape[1])
    logit_scale = sd.pop("logit_scale")
    tower.load_state_dict(sd)
    tower.logit_scale = nn.Parameter(logit_scale.reshape(()))      # what VLSA adopts next to the tower (model/vlsa.py:105)
    return tower

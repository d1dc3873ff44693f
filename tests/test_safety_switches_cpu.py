"""CPU side of the safety net: the environment switches are parsed once at import, the look-ahead / deferral state
follows re-assigned encoder parameters (structure epoch) and plain scalar attributes, the structure hooks are installed by the first
model and not at import, the PARANOID comparison raises on a mismatch (stubbed per-bag route: no device here), and which event changes
which of the model's keys (a table that holds before and after the keys were rebuilt on ``vlsa_amd.model_state``)."""
import subprocess
import sys

import pytest
import torch


def test_env_switches_are_read_at_import():
    code = ("import vlsa_amd.vlsa as V; print(int(V.ENV_NO_DEFER), int(V.ENV_NO_LOOKAHEAD), int(V.ENV_PARANOID), "
            "int(getattr(V._install_structure_hooks, 'done', False)))")
    import os
    env = dict(os.environ, VLSA_AMD_NO_DEFER="1", VLSA_AMD_NO_LOOKAHEAD="0", VLSA_AMD_PARANOID="yes")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(__file__)))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "0", "1", "0"]      # ... and importing the module installed no process-global hook


def _net(P=4, K=3):
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="VLFAN", dim_in=512, use_feat_proj=False, query="Parameter", num_query=P, query_pooling="mean")
    return VLSA.from_modules(cfg, pretrained_text_features=torch.randn(K, 512, generator=torch.Generator().manual_seed(1)))


def test_first_model_installs_the_structure_hooks_and_state_follows_reassignment():
    from vlsa_amd import vlsa as V
    net = _net()
    assert V._HOOKS_INSTALLED[0]
    T = net._text_features()
    s0 = net._eval_state(T)
    assert net._same_state(s0, net._eval_state(T))
    enc = net.mil_encoder
    enc.Q = torch.nn.Parameter(enc.Q.detach().clone())                       # a new object with the same version (0) as the old one
    s1 = net._eval_state(T)
    assert not net._same_state(s0, s1)                                        # the kept lists were re-walked (structure epoch)
    enc.query_pooling = "max"                                                 # a plain attribute
    s2 = net._eval_state(T)
    assert not net._same_state(s1, s2) and net._same_state(s2, net._eval_state(T))
    k0 = net._defer_key()
    enc.query_pooling = "mean"
    assert net._defer_key() != k0


def test_paranoid_check_raises_on_a_mismatch(monkeypatch):
    from vlsa_amd import vlsa as V
    net = _net()
    ref = torch.tensor([[1.0, 2.0, 3.0]])
    monkeypatch.setattr(net, "forward", lambda X: (ref.clone(), None, None))
    X = torch.zeros(1, 5, 512)
    assert net._paranoid_check(X, ref[0] + 5e-5, "stub") < V.PARANOID_TOLERANCE
    with pytest.raises(V.ParanoidMismatch, match="per-bag route"):
        net._paranoid_check(X, ref[0] + 1e-3, "stub")
    assert net._paranoid_checks == 2 and net._materialising is False


def test_identity_featmil_is_never_deferred():
    from vlsa_amd.vlsa import VLSA
    net = VLSA.from_modules(dict(name="FeatMIL", dim_in=512, pooling="logit_top10"),
                            pretrained_text_features=torch.randn(3, 512, generator=torch.Generator().manual_seed(2)))
    net.train()
    net.defer_training_calls = True

    class FakeCuda(torch.Tensor):          # `takes` wants a device tensor: stand in for one on the CPU
        is_cuda = True
    X = torch.zeros(1, 7, 512).as_subclass(FakeCuda)
    assert net._defer_call(X, torch.zeros(3, 512)) is None


def _keys(net, T):
    return net._provider_key(), net._eval_state(T), net._defer_key()


def _changed(net, before, after):
    return (before[0] != after[0], not net._same_state(before[1], after[1]), before[2] != after[2])


def test_the_four_keys_through_a_scripted_sequence_of_mutations():
    """Which of ``_provider_key`` / ``_eval_state`` + ``_same_state`` / ``_defer_key`` each event changes -- the table below, written
    from the rules (what each key depends on), is the same before and after the keys were rebuilt on ``ModuleWatch``: this test reads
    the keys through those method names only (its events also call ``forward_text_only`` and ``load_state_dict``, the occasions of an
    exact walk that need no device) and passes unchanged on the commit before.  One thing the table cannot show: that commit's ``_defer_key``
    held the VERSIONS of the encoder's tensors but not their identity, so the re-assigned ``enc.Q`` below changes it there only because
    the old ``Q`` had been written in place (version 1 against 0); it now changes for a same-version replacement too
    (``test_model_state_cpu.py::test_defer_key_sees_a_same_version_replacement``)."""
    import torch.nn as nn
    from test_text_cache_cpu import Learner, Tower
    from vlsa_amd.vlsa import VLSA
    torch.manual_seed(0)
    tower, learner = Tower(), Learner()
    cfg = dict(name="VLFAN", dim_in=512, use_feat_proj=False, query="Parameter", num_query=4, query_pooling="mean")
    net = VLSA.from_modules(dict(cfg), prompt_learner=learner, prompt_encoder=tower).eval()
    fixed = VLSA.from_modules(dict(cfg), pretrained_text_features=torch.randn(3, 512)).eval()
    enc = net.mil_encoder
    T0, T1 = torch.randn(3, 512), torch.randn(3, 512)
    text, ctx = [T0], []

    def swap(obj, name, value):
        setattr(obj, name, value)

    def no_grad_on():
        ctx.append(torch.no_grad())
        ctx[-1].__enter__()

    def no_grad_off():
        ctx.pop().__exit__(None, None, None)

    spare = [nn.Parameter(torch.randn(512, 8)), nn.Parameter(torch.zeros(2)), nn.Parameter(torch.randn(4, 512)), torch.ones([]) * 4.0]

    def miss(sub, name, value):
        if value is None:
            delattr(tower, name)
        else:
            getattr(tower, sub)._parameters[name] = value
        learner.context_embeds.detach().add_(0.25)
        net.forward_text_only()

    def reload():
        enc._parameters["Q"] = spare[2]
        enc.coattn_logit_scale = spare[3]                     # (a plain tensor attribute: no registration)
        net.load_state_dict(net.state_dict())

    ALL = (True, True, True)
    P, E, D = (True, False, True), (False, True, True), (False, False, True)           # provider side / encoder side / defer key only
    NONE, EVAL = (False, False, False), (False, True, False)
    script = [
        # (model, event, what it does, (provider key, eval state, defer key) changed)
        (net, "nothing", lambda: None, NONE),
        (net, "in-place write, tower weight", lambda: tower.blocks[1][0].weight.detach().mul_(1.5), P),
        (net, "in-place write, learner parameter", lambda: learner.context_embeds.detach().add_(0.25), P),
        (net, "in-place write, learner buffer", lambda: learner.pseudo_sentence_tokens.add_(1), P),
        (net, "in-place write, encoder query", lambda: enc.Q.detach().add_(0.1), E),
        (net, "in-place write, logit scale", lambda: net.logit_scale.detach().add_(0.1), E),
        (net, "in-place write, co-attention scale", lambda: enc.coattn_logit_scale.add_(0.1), E),
        (net, "learner parameter re-assigned (same version)",
         lambda: swap(learner, "context_embeds", nn.Parameter(torch.randn(3, 5, 8))), P),
        (net, "tower submodule re-assigned", lambda: swap(tower, "proj", nn.Linear(8, 512)), P),
        (net, "learner buffer re-assigned", lambda: swap(learner, "pseudo_sentence_tokens", torch.ones(3, 5, dtype=torch.long)), P),
        (net, "encoder query re-assigned", lambda: swap(enc, "Q", nn.Parameter(enc.Q.detach().clone())), E),
        (net, "logit scale re-assigned", lambda: swap(net, "logit_scale", nn.Parameter(torch.ones([]) * 2.0)), E),
        (net, "a module is built elsewhere", lambda: nn.Linear(3, 3), NONE),
        (net, "dropout deep in the tower to train", lambda: tower.blocks[2][1].train(), P),
        (net, "encoder to train", lambda: enc.train(), E),
        (net, "grad mode off", no_grad_on, P),
        (net, "grad mode on again", no_grad_off, P),
        (net, "self.training", lambda: swap(net, "training", True), D),
        (net, "plain attribute query_pooling", lambda: swap(enc, "query_pooling", "max"), E),
        (net, "plain attribute keep_ratio", lambda: swap(enc, "keep_ratio", 0.25), E),
        (net, "image_encoder_cfg['pooling']", lambda: net.image_encoder_cfg.__setitem__("pooling", "logit_top5"), E),
        (net, "another text-feature tensor", lambda: text.__setitem__(0, T1), EVAL),
        (net, "in-place write to the text features", lambda: T1.add_(1.0), EVAL),
        (net, "nothing, again", lambda: None, NONE),
        # what is no registration is seen by the exact walk of the next text-cache miss / load_state_dict at the latest: the row after
        # each one writes to the object that only such a walk can have found (or lost) -- no module is built in between
        (net, "a parameter written into tower._parameters, then a text-cache miss", lambda: miss("proj", "weight", spare[0]), P),
        (net, "in-place write to that parameter", lambda: spare[0].detach().mul_(0.5), P),
        (net, "a spare tower parameter registered", lambda: swap(tower, "spare", spare[1]), P),
        (net, "del tower.spare, then a text-cache miss", lambda: miss(None, "spare", None), P),
        (net, "in-place write to the deleted parameter", lambda: spare[1].detach().add_(1.0), NONE),
        (net, "enc._parameters['Q'] written, plain-attribute co-attention scale re-assigned, then load_state_dict", reload, ALL),
        (net, "in-place write to that query", lambda: spare[2].detach().add_(0.1), E),
        (net, "in-place write to that co-attention scale", lambda: spare[3].add_(0.1), E),
        (fixed, "nothing", lambda: None, NONE),
        (fixed, "in-place write, fixed text buffer", lambda: fixed.pretrained_text_features.add_(1.0), D),
        (fixed, "fixed text buffer re-assigned", lambda: swap(fixed, "pretrained_text_features", torch.randn(3, 512)), D),
        (fixed, "in-place write, encoder query", lambda: fixed.mil_encoder.Q.detach().add_(0.1), E),
    ]
    assert fixed._provider_key() is None                            # nothing to see into and nothing needed: the buffer is the text side
    wrong = []
    for model, event, act, expect in script:
        before = _keys(model, text[0])
        act()
        got = _changed(model, before, _keys(model, text[0]))
        if got != expect:
            wrong.append((event, got, expect))
    assert not wrong, wrong

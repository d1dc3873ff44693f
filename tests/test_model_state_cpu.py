"""vlsa_amd/model_state.py: the kept walk (``ModuleWatch``) behind every cache key of the drop-in model, alone on small trees; and a
model that carries the transient names of the version before the watches existed.  (Which event changes which of the model's keys:
the table in tests/test_safety_switches_cpu.py.)"""
import copy
import io
import os
import subprocess
import sys

import torch
import torch.nn as nn

from vlsa_amd import model_state
from vlsa_amd.model_state import ModuleWatch
from vlsa_amd.vlsa import VLSA

from test_text_cache_cpu import Learner, Tower


def _tree():
    return nn.Sequential(nn.Linear(4, 4), nn.Sequential(nn.Linear(4, 4), nn.Dropout(0.5)), nn.BatchNorm1d(4))


def test_stamp_follows_versions_flags_and_reassignment():
    m, w = _tree(), ModuleWatch()
    s0 = w.stamp(m)
    assert isinstance(hash(s0), int) and w.stamp(m) == s0
    with torch.no_grad():
        m[0].weight.mul_(2.0)                                       # in-place write to a parameter ...
    s1 = w.stamp(m)
    assert s1 != s0
    m[2].running_mean.add_(1.0)                                     # ... and to a buffer
    s2 = w.stamp(m)
    assert s2 != s1
    m[1][1].eval()                                                  # the flag of one submodule deep in the tree
    s3 = w.stamp(m)
    assert s3 != s2 and w.stamp(m) == s3
    m[0].bias = old = nn.Parameter(torch.zeros(4))
    s3 = w.stamp(m)
    m[0].bias = nn.Parameter(torch.zeros(4))                        # re-assigned parameter with the old one's version
    assert m[0].bias._version == old._version
    s4 = w.stamp(m)
    assert s4 != s3 and any(t is m[0].bias for t in w.lists()[1]) and not any(t is old for t in w.lists()[1])
    m[2].running_var = torch.ones(4)                                # re-assigned buffer
    s5 = w.stamp(m)
    assert s5 != s4
    m[1][0] = nn.Linear(4, 4)                                       # re-assigned submodule
    s6 = w.stamp(m)
    assert s6 != s5 and any(x is m[1][0] for x in w.lists()[0])
    other = _tree()                                                 # another module object: walked, a stamp of its own
    assert w.stamp(other) != s6 and w.module is other


def test_generation_survives_an_identical_walk_and_a_registration_elsewhere(monkeypatch):
    m, w = _tree(), ModuleWatch()
    walks = []
    orig = model_state._walk_module
    monkeypatch.setattr(model_state, "_walk_module", lambda x: (walks.append(x), orig(x))[1])
    s0 = w.stamp(m)
    gen = w.generation
    assert len(walks) == 1 and w.stamp(m) == s0 and w.stamp(m) == s0 and len(walks) == 1       # steady state: no walk at all
    nn.Linear(3, 3)                                                 # somebody builds a module: walked again, the same objects
    assert w.stamp(m) == s0 and len(walks) == 2 and w.generation == gen
    assert w.stamp(m, exact=True) == s0 and len(walks) == 3 and w.generation == gen
    w.forget()
    assert w.lists()[0] and w.stamp(m) == s0 and len(walks) == 4 and w.generation == gen
    assert w.stamp(m) == s0 and len(walks) == 4
    m[0].weight = nn.Parameter(m[0].weight.detach().clone())        # a swapped object: a fresh generation, never handed out before
    assert w.stamp(m) != s0 and w.generation > gen
    w2 = ModuleWatch()
    w2.stamp(_tree())
    assert w2.generation > w.generation


def test_changes_that_are_no_registration_are_seen_by_the_next_exact_walk():
    m, w = _tree(), ModuleWatch()
    s0 = w.stamp(m)
    old = m[0].weight
    m[0]._parameters["weight"] = nn.Parameter(old.detach().clone())           # a write into the dict: no hook runs
    assert w.stamp(m, exact=True) != s0 and not any(t is old for t in w.lists()[1])
    s1 = w.stamp(m)
    del m[0].bias
    w.forget()
    s2 = w.stamp(m)
    assert s2 != s1 and len(s2[3]) == len(s1[3]) - 1


def test_shared_submodule_once_and_extra_tensors():
    shared = nn.Linear(4, 4)
    m = nn.Sequential(nn.Sequential(shared), nn.Sequential(shared, nn.ReLU()))
    extra = [torch.zeros(2)]                                        # the owner handed to every stamp: the watch keeps no reference to it
    w = ModuleWatch(lambda owner: list(owner))
    s0 = w.stamp(m, False, extra)
    sub, tensors = w.lists()
    assert sum(1 for x in sub if x is shared) == 1 and len(sub) == 5
    assert sum(1 for t in tensors if t is shared.weight) == 1 and len(tensors) == 3 and tensors[-1] is extra[0]
    extra[0].add_(1.0)                                              # an extra tensor's version is in the stamp
    s1 = w.stamp(m, False, extra)
    assert s1 != s0
    extra[0] = torch.zeros(2)                                       # a re-assigned extra: no registration, the next exact walk sees it
    assert w.stamp(m, True, extra) != s1 and w.lists()[1][-1] is extra[0]


def test_no_hook_before_the_first_stamp():
    code = ("import torch.nn as nn\nfrom vlsa_amd import model_state as S\nw = S.ModuleWatch()\nm = nn.Linear(2, 2)\n"
            "a = S._HOOKS_INSTALLED[0]\nw.stamp(m)\nprint(int(a), int(S._HOOKS_INSTALLED[0]))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "1"]


# -- the keys of the model on top of it (their table of events: tests/test_safety_switches_cpu.py) ----------------------------------
_CFG = dict(name="VLFAN", dim_in=512, use_feat_proj=False, query="Parameter", num_query=4, query_pooling="mean")


def test_defer_key_sees_a_same_version_replacement():
    net = VLSA.from_modules(dict(_CFG), pretrained_text_features=torch.randn(3, 512)).eval()
    k0 = net._defer_key()
    old = net.mil_encoder.Q
    net.mil_encoder.Q = nn.Parameter(old.detach().clone())
    assert net.mil_encoder.Q._version == old._version and net._defer_key() != k0


def test_a_new_window_an_extension_and_a_new_deferred_batch_walk_the_encoder_exactly():
    """The three occasions of an exact walk that a device normally stands behind, with the device part stubbed: each must find a
    parameter written into ``enc._parameters`` (no registration: no hook ran)."""
    net = VLSA.from_modules(dict(_CFG), pretrained_text_features=torch.randn(3, 512)).eval()
    T, enc = net._text_features(), net.mil_encoder
    watched = lambda t: any(x is t for x in net._get_watches()["mil_encoder"].lists()[1])        # noqa: E731

    class Resident(list):                                            # stands in for a ResidentBags dataset of three items
        def resident_view(self, i):
            return self[i]
    X = torch.zeros(5, 512)
    rb = Resident([X, X, X])
    net._lookahead_window = lambda la, T, width: 0                   # (the batched launch: nothing to run here)
    s0 = net._eval_state(T)
    enc._parameters["Q"] = q1 = nn.Parameter(enc.Q.detach().clone())
    assert net._same_state(s0, net._eval_state(T)) and not watched(q1)           # not seen without an exact walk ...
    assert net._lookahead((rb, 0), X[None], T) is None and watched(q1)           # ... a new window asks for one
    assert not net._same_state(s0, net._la["state"])
    enc._parameters["Q"] = q2 = nn.Parameter(enc.Q.detach().clone())
    la = dict(net._la, hi=0, last=0, rows={})
    net._lookahead_extend(la, T)                                     # the extension: walks, finds another state, launches nothing
    assert watched(q2) and la["state"] is net._la["state"]
    enc._parameters["Q"] = q3 = nn.Parameter(enc.Q.detach().clone())

    class FakeCuda(torch.Tensor):                                    # `takes` wants a device tensor: stand in for one on the CPU
        is_cuda = True
    net.train()
    assert net._defer_call(X[None].as_subclass(FakeCuda), T) is not None and watched(q3)
    assert any(t is q3 for t in net._pending_calls.trainable)


def test_a_dropped_model_is_freed_without_the_cycle_collector():
    """The watches live in the model and must not point back at it: a model dropped by its last reference frees its weights (and, on
    the device, its plans and look-ahead rows) at once -- the cycle collector gets no pressure signal from device memory."""
    import gc
    import weakref
    was = gc.isenabled()
    gc.disable()
    try:
        net = VLSA.from_modules(dict(_CFG), pretrained_text_features=torch.randn(3, 512)).eval()
        T = net._text_features()
        net._eval_state(T, exact=True), net._defer_key(), net._provider_key()
        assert "_watches" in net.__dict__ and net._get_watches()["mil_encoder"].lists()[1][-2] is net.logit_scale
        ref = weakref.ref(net)
        del net
        assert ref() is None
    finally:
        if was:
            gc.enable()


def test_a_non_plain_scalar_enters_the_state_by_identity():
    net = VLSA.from_modules(dict(_CFG), pretrained_text_features=torch.randn(3, 512)).eval()
    T, enc = net._text_features(), net.mil_encoder
    enc.keep_ratio = a = torch.tensor([0.5, 0.5])                   # (a multi-element tensor: `==` on it would be elementwise)
    s0, k0 = net._eval_state(T), net._defer_key()
    assert isinstance(hash(s0[0]), int) and net._same_state(s0, net._eval_state(T)) and net._defer_key() == k0
    enc.keep_ratio = torch.tensor([0.5, 0.5])                       # another object of equal value: not the same state
    assert not net._same_state(s0, net._eval_state(T)) and net._defer_key() != k0
    enc.keep_ratio = a
    assert net._same_state(s0, net._eval_state(T)) and net._defer_key() == k0


def test_each_invalidation_level_clears_exactly_its_row_of_the_table():
    from vlsa_amd import vlsa as V

    def filled():
        net = VLSA.from_modules(dict(_CFG), prompt_learner=Learner(), prompt_encoder=Tower()).eval()
        with torch.no_grad():
            net.forward_text_only()
        net._eval_state(net._text_cache)
        net._la, net._hot["h"], net._plans["p"], net._train_plans["t"] = {"rows": {}}, 1, 2, 3
        net._prepared_text = net._prepared_query = torch.zeros(1)
        return net

    def left(net):
        fresh = all(w.epoch == -1 for w in net._get_watches().values())
        return dict(la=net._la is not None, text=net._text_cache is not None and net._text_cache_key is not None, watches=not fresh,
                    hot=bool(net._hot), plans=bool(net._plans), train_plans=bool(net._train_plans),
                    prepared=net._prepared_text is not None and net._prepared_query is not None)
    everything = dict(la=True, text=True, watches=True, hot=True, plans=True, train_plans=True, prepared=True)
    assert left(filled()) == everything
    net = filled()
    net._invalidate(V._FORWARD)
    assert left(net) == dict(everything, la=False)
    for act in (lambda n: n._invalidate(V._WEIGHTS), lambda n: n.load_state_dict(n.state_dict())):
        net = filled()
        act(net)
        assert left(net) == dict(everything, la=False, text=False, watches=False, hot=False)
    for act in (lambda n: n._invalidate(V._STORAGE), lambda n: n.float()):
        net = filled()
        act(net)
        assert left(net) == dict.fromkeys(everything, False)


def test_a_model_with_the_earlier_transient_names_loads_and_works():
    """A model pickled before the watches existed carries ``_provider_lists`` / ``_la_lists`` in its ``__dict__`` and no ``_watches``."""
    torch.manual_seed(0)
    net = VLSA.from_modules(dict(_CFG), prompt_learner=Learner(), prompt_encoder=Tower()).eval()
    with torch.no_grad():
        a = net.forward_text_only().clone()
    net.__dict__["_provider_lists"], net.__dict__["_la_lists"] = {}, None
    net.__dict__.pop("_watches", None)
    twin = copy.deepcopy(net)
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    for m in (twin, back):
        assert "_watches" not in m.__dict__ and m.__dict__["_provider_lists"] == {} and m.__dict__["_la_lists"] is None
        with torch.no_grad():
            T = m.forward_text_only()
            assert torch.equal(T, a) and m.forward_text_only() is T
            s0 = m._eval_state(T)
            assert m._same_state(s0, m._eval_state(T))
            m.mil_encoder.Q.add_(1.0)
            assert not m._same_state(s0, m._eval_state(T))
        assert m._get_watches()["prompt_encoder"].module is m.prompt_encoder

"""What a cached result of the drop-in model depends on besides the bag: ONE mechanism behind every cache key of ``vlsa_amd.vlsa``
(text cache, look-ahead windows, hot call, deferred training calls).  Pure Python, no native calls.

A ``ModuleWatch`` keeps the walk of one module tree -- its submodules, its parameters + buffers, optional extra tensors that are not
registered in the tree -- and hands out ``stamp(module)``: a hashable tuple that is equal exactly as long as the tree holds the same
objects, with the same train / eval flags and the same in-place versions.  The rules, stated once:

  in-place write to a watched tensor .............. its ``_version`` is in the stamp
  train / eval flag of any submodule .............. in the stamp
  parameter / buffer / submodule re-assigned ...... torch's global registration hooks bump the structure epoch (``module.x =
                                                    nn.Parameter(...)`` goes through them): the next stamp re-walks, finds another
                                                    object and takes a fresh generation (versions alone cannot tell a re-assigned
                                                    parameter from the old one)
  a registration anywhere else in the process ..... re-walks too, finds the same objects (``is``, position by position), keeps its
                                                    generation: the stamp is unchanged
  ``del m.weight``, ``m._parameters[...] = ``,      not registrations: seen by the next EXACT walk -- ``stamp(module, exact=True)`` or
  a re-assigned extra tensor                        the first stamp after ``forget()`` -- which the callers ask for on every cache
                                                    miss, new look-ahead window, window extension and new deferred batch
  steady state .................................... no walk: two C-level ``map(attrgetter)`` loops over the kept lists

A stamp never holds the ``id()`` of an object the watch does not keep alive (a freed object's address is handed out again): the
watch holds strong references to the module and to everything of the last walk, and a generation is never handed out twice.

SIDE EFFECT: the hooks are process-global -- one Python callback per registration in ANY model of the process --
and are installed when the first ``VLSA`` is assembled or, for a model unpickled in a fresh process (it never runs ``_assemble``), by
the first stamp; not at import."""
from __future__ import annotations

import operator

_GET_TRAINING, _GET_VERSION = operator.attrgetter("training"), operator.attrgetter("_version")
_STRUCT_EPOCH = [0, 0]          # [registrations seen, generations handed out]
_HOOKS_INSTALLED = [False]


def _bump_structure_epoch(*_args, **_kwargs):
    _STRUCT_EPOCH[0] += 1
    return None


def _install_structure_hooks():
    """Idempotent."""
    if _HOOKS_INSTALLED[0]:
        return
    _HOOKS_INSTALLED[0] = True
    _STRUCT_EPOCH[0] += 1          # lists walked before the hooks existed are not trusted
    from torch.nn.modules import module as _m
    _m.register_module_parameter_registration_hook(_bump_structure_epoch)
    _m.register_module_buffer_registration_hook(_bump_structure_epoch)
    _m.register_module_module_registration_hook(_bump_structure_epoch)


def _walk_module(m):
    """(submodules, parameters + buffers) of a module tree, dict order, every object once (nn.Module.parameters() spends
    ~0.3 ms on a 150-tensor text tower in generator / prefix-string bookkeeping)."""
    sub, tensors, stack, seen = [], [], [m], set()
    while stack:
        x = stack.pop()
        if id(x) in seen:
            continue
        seen.add(id(x))
        sub.append(x)
        tensors.extend(t for t in x._parameters.values() if t is not None)
        tensors.extend(t for t in x._buffers.values() if t is not None)
        stack.extend(c for c in x._modules.values() if c is not None)
    return sub, tensors


class ModuleWatch:
    """The kept walk of one module tree.  ``extras``: a function of the ``owner`` handed to ``stamp`` giving the tensors outside the
    tree that belong to the stamp (read again at every walk), or None.  The watch holds no reference to the owner: a model that keeps
    its watches is still freed by its last reference, without the cycle collector."""

    __slots__ = ("extras", "module", "submodules", "tensors", "epoch", "generation")

    def __init__(self, extras=None):
        self.extras, self.module, self.submodules, self.tensors, self.epoch, self.generation = extras, None, [], [], -1, 0

    def stamp(self, module, exact=False, owner=None):
        if exact or module is not self.module or self.epoch != _STRUCT_EPOCH[0]:
            self._walk(module, owner)
        return (id(module), self.generation, tuple(map(_GET_TRAINING, self.submodules)), tuple(map(_GET_VERSION, self.tensors)))

    def _walk(self, module, owner):
        _install_structure_hooks()
        sub, tensors = _walk_module(module)
        if self.extras is not None:
            tensors += self.extras(owner)
        if not (module is self.module and len(sub) == len(self.submodules) and len(tensors) == len(self.tensors)
                and all(map(operator.is_, sub, self.submodules)) and all(map(operator.is_, tensors, self.tensors))):
            _STRUCT_EPOCH[1] += 1
            self.generation = _STRUCT_EPOCH[1]
        self.module, self.submodules, self.tensors, self.epoch = module, sub, tensors, _STRUCT_EPOCH[0]

    def lists(self):
        """(submodules, tensors) of the last walk; empty before the first stamp"""
        return self.submodules, self.tensors

    def forget(self):
        """the next stamp walks (and keeps its generation if it finds what the last walk found)"""
        self.epoch = -1

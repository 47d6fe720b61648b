"""The one protocol behind every cache of weight-derived operands: bf16 copies of parameters, PackedWeight images, the mixers' derived
tensors, the fused inference path's bundles.  An entry is a ``(key, value)`` pair under its kind's attribute on its owner (a parameter
or a module); keys are tuples of ``(parameter version, storage pointer)`` pairs, compared as such.  A kind is declared once, next to the
code that builds its values; ``Kind.lookup`` alone decides between hit, refresh in place and allocate; ``rekey_caches`` and
``invalidate_caches`` walk the declared kinds.

Under hipGraph replay (brain.Brain graph_steps) a captured launch reads a cached tensor by ADDRESS, so the kinds a training graph reads
(``graphs_read``) must keep their storage for as long as a graph lives and be refreshed in place:
  CACHE_INPLACE     a miss that finds an older entry its kind calls reusable rewrites that entry's storage instead of allocating
  CACHE_GENERATION  bumped whenever such an entry gets NEW storage or entries are dropped: graphs captured before the bump may hold
                    addresses the caches no longer own (brain drops them); CM_CACHE_TRACE=1 prints the call chain of every bump
  forced_refresh()  context: every entry's FIRST lookup is treated as a miss (while the "fresh" variant of a graph is captured: the
                    refresh kernels land in the graph) and (owner, attribute) of every refreshed entry is collected, so that the keys
                    of exactly those entries can be brought up to date after a replay did the refresh (rekey_caches) -- Python does
                    not see a replay's kernels
The other kinds (fused.py's inference bundles) are rebuilt on a miss and take no part in this: an evaluation pass between training
epochs must not make brain drop its captured graphs.
"""
from __future__ import annotations

import contextlib
import os

CACHE_INPLACE = False
CACHE_GENERATION = 0
_FORCE = None                                     # None, or the set of (id(owner), attribute) already refreshed in this forced pass
_LOG = None
_KINDS = {}                                       # attribute -> Kind


@contextlib.contextmanager
def forced_refresh():
    global _FORCE, _LOG
    old = (_FORCE, _LOG)
    _FORCE, _LOG = set(), []
    try:
        yield _LOG
    finally:
        _FORCE, _LOG = old


def _new_storage():
    global CACHE_GENERATION
    CACHE_GENERATION += 1
    if os.environ.get("CM_CACHE_TRACE"):                              # who allocates: one line per bump
        import traceback
        print("cache generation", CACHE_GENERATION, " <- ".join(f"{f.name}:{f.lineno}" for f in traceback.extract_stack()[-6:-1]), flush=True)


def _note(owner, attr):
    if _FORCE is not None:
        _FORCE.add((id(owner), attr))
        _LOG.append((owner, attr))


class Kind:
    """``attr``: the attribute the entries live under.  ``graphs_read``: see above; such a kind gives ``key_of(owner, value)``, the entry's
    current key from the owner's parameters and what the value records of the rest (its dtype).  With ``args`` what lookup() got:
    ``build(owner, *args)`` makes a value; ``usable(old, owner, *args)``: the old value can answer this lookup at all (None: any can);
    ``reusable(old, owner, *args)``: it can moreover be rewritten in place (None: any usable one), by ``refresh_(old, owner, *args)``."""

    def __init__(self, attr, graphs_read, build, key_of=None, usable=None, reusable=None, refresh_=None):
        self.attr, self.graphs_read, self.build, self.key_of = attr, graphs_read, build, key_of
        self.usable, self.reusable, self.refresh_ = usable, reusable, refresh_
        assert not graphs_read or (key_of is not None and refresh_ is not None), "a kind that graphs read is refreshed in place and re-keyed"
        _KINDS[attr] = self

    def lookup(self, owner, key, *args):
        """The value for ``key``: the only code that decides between hit, refresh in place and allocate."""
        attr, tracked = self.attr, self.graphs_read
        c = getattr(owner, attr, None)
        ok = c is not None and (self.usable is None or self.usable(c[1], owner, *args))
        if ok and c[0] == key and not (tracked and _FORCE is not None and (id(owner), attr) not in _FORCE):
            return c[1]
        if tracked and CACHE_INPLACE and ok and self.refresh_ is not None and (self.reusable is None or self.reusable(c[1], owner, *args)):
            self.refresh_(c[1], owner, *args)                         # same storage, new values
            # the key as it is NOW: a value "in the compute dtype" may alias its fp32 parameter, and writing it moved the version
            setattr(owner, attr, (self.key_of(owner, c[1]), c[1]))
            _note(owner, attr)
            return c[1]
        value = self.build(owner, *args)
        try:
            setattr(owner, attr, (key, value))
            if tracked:
                _new_storage()
                _note(owner, attr)
        except (AttributeError, RuntimeError):                        # an owner that takes no attributes: served uncached
            pass
        return value


def param_key(p, value=None):
    """Key of an entry derived from ONE tensor.  data_ptr: `p.data = ...` swaps storage without bumping _version."""
    return (p._version, p.data_ptr())


def module_params(m):
    """m's parameter OBJECTS, listed once (Module.parameters() walks the module tree: 3 ms of host time per training step, which is
    host-bound); invalidate_caches drops the list."""
    pl = m.__dict__.get("_cm_plist")
    if pl is None:
        pl = m.__dict__["_cm_plist"] = list(m.parameters())
    return pl


def rekey_caches(entries) -> None:
    """entries: what forced_refresh() collected.  Marks each entry as holding the CURRENT version of its parameter(s): call only
    right after the kernels that refresh exactly these entries ran (a replay of the graph they were captured into)."""
    for owner, attr in entries:
        c = getattr(owner, attr, None)
        if c is not None:
            setattr(owner, attr, (_KINDS[attr].key_of(owner, c[1]), c[1]))


def invalidate_caches(module) -> None:
    """Drop every cached weight-derived operand under ``module`` (every declared kind, on its parameters and its submodules).
    The caches key on (parameter version, storage pointer): in-place writes made under torch.no_grad() on the parameter itself,
    optimizer steps, load_state_dict and `p.data = new` are seen; writes THROUGH ``p.data`` (``p.data.copy_()``, EMA / SWA code,
    vector_to_parameters) are not -- call this after them.  Nor is a parameter OBJECT replaced on a mixer module
    (``m.in_proj.weight = nn.Parameter(...)``, as opposed to its data): the mixers' derived operands key on the parameter list
    module_params() memoised, which still holds the old object -- call this after that too.
    load_state_dict calls it by itself (hook installed by asr.ConMambaASR)."""
    _new_storage()
    # entries are plain attributes, so they sit in the owner's __dict__ (a Parameter has one; an owner that took no attribute, see
    # lookup, holds no entry)
    for owner in (*module.parameters(), *module.modules()):
        for attr in ("_cm_plist", *_KINDS):
            owner.__dict__.pop(attr, None)

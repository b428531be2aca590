"""Host-side caching shared by the drop-in modules (AEI_Net, IResNet).

* ``PackedModule``: a module whose weights are packed once per (device, compute dtype) into the
  kernels' layouts.  The pack is reused until one of these invalidates it:
  - the key (device, dtype) changes;
  - ``load_state_dict`` runs;
  - ``_apply`` (``.to`` / ``.cuda`` / ``.half`` ...) runs on the module **or on any of its submodules**
    (every submodule's ``_apply`` is wrapped at construction to invalidate its owner);
  - a parameter, buffer or submodule is assigned anew anywhere in the tree (``m.weight = nn.Parameter(...)``,
    ``m.register_buffer(...)``: torch's global registration hooks, filtered to modules this tree owns);
  - a parameter or buffer is modified in place (its version counter moved: one C-level pass over the cached
    tensors' counters, ~30 us for AEI_Net's 311 tensors, not a ``state_dict()`` walk ~0.9 ms).
  Not detected: swapping a tensor's storage with ``p.data = t`` (no version bump, no hook); call
  ``invalidate_pack()`` after doing that.
* ``WorkspaceCache``: one device workspace per (mode, batch, stream), reused by later calls on the
  same stream.  Launches on one stream are ordered, so a call never overwrites scratch that an
  earlier call still reads; two streams (two batches in flight) get two workspaces.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import operator
import types
import weakref
from typing import Callable

import numpy as np
import torch
import torch.nn as nn
import torch.nn.modules.module as _tmod

from . import _lib

_VERSION = operator.attrgetter("_version")
_OWNER = "_ghost_pack_owner"


def _owner_of(module):
    ref = module.__dict__.get(_OWNER)
    return ref() if ref is not None else None


def _on_register(module, name, value):
    """Global registration hook: a parameter / buffer / submodule assigned into a module of a packed tree."""
    root = _owner_of(module)
    if root is not None:
        root._invalidate()
        if isinstance(value, nn.Module):
            root._adopt(value)
    return None


def _owned_apply(self, fn, *args, **kwargs):
    """``_apply`` of a submodule of a packed tree (``.to`` / ``.half`` on the submodule itself)."""
    root = _owner_of(self)
    if root is not None:
        root._invalidate()
    return type(self)._apply(self, fn, *args, **kwargs)


_HOOKS_INSTALLED = False


def _install_hooks():
    global _HOOKS_INSTALLED
    if not _HOOKS_INSTALLED:
        _tmod.register_module_parameter_registration_hook(_on_register)
        _tmod.register_module_buffer_registration_hook(_on_register)
        _tmod.register_module_module_registration_hook(_on_register)
        _HOOKS_INSTALLED = True


class PackedModule(nn.Module):
    def _init_packed(self):
        self._rt = None
        self._rt_key = None        # (device, compute dtype) the runtime was packed for
        self._rt_tensors = ()      # the state_dict tensors it was packed from, and their version counters
        self._rt_versions = ()
        self.register_load_state_dict_post_hook(lambda module, keys: module._invalidate())
        _install_hooks()
        for m in self.modules():
            if m is not self:
                self._adopt(m)

    def _adopt(self, m: nn.Module):
        """Mark m (and its subtree) as owned by this packed module: assignments into it and ``m.to(...)`` /
        ``m.half()`` invalidate the pack."""
        ref = weakref.ref(self)
        for sub in m.modules():
            if sub is self:
                continue
            sub.__dict__[_OWNER] = ref
            if "_apply" not in sub.__dict__:
                # a bound method (deepcopy rebinds it to the copy), not a closure over this instance
                sub.__dict__["_apply"] = types.MethodType(_owned_apply, sub)

    def _invalidate(self):
        self._rt_key = None

    def invalidate_pack(self):
        """Force a re-pack on the next call (after ``p.data = t``, which nothing can observe cheaply)."""
        self._invalidate()

    def _apply(self, fn, *args, **kwargs):
        if hasattr(self, "_rt_key"):
            self._invalidate()
        return super()._apply(fn, *args, **kwargs)

    def _pack_current(self, rt=None) -> bool:
        """True when the cached pack (and, if given, exactly the runtime ``rt``) is still valid."""
        return (self._rt is not None and self._rt_key is not None and (rt is None or self._rt is rt)
                and tuple(map(_VERSION, self._rt_tensors)) == self._rt_versions)

    def _cached_runtime(self, device, dt, build: Callable[[dict], object]):
        """The runtime for (device, dt); ``build(state_dict)`` packs a new one when stale."""
        if self._rt_key == (device, dt) and self._pack_current():
            return self._rt
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        for k, v in sd.items():
            if v.is_floating_point() and v.device != device:
                raise RuntimeError(f"ghost_amd: parameter {k} is on {v.device}, input on {device}")
        self._rt = None     # release the previous handle (and its workspaces) before allocating anew
        with torch.no_grad():
            self._rt = build(sd)
        self._rt_key = (device, dt)
        self._rt_tensors = tuple(self.state_dict().values())
        self._rt_versions = tuple(map(_VERSION, self._rt_tensors))
        return self._rt


class WorkspaceCache:
    """At most ``cap`` workspaces, least recently used evicted (each was allocated while its stream was
    current, so the caching allocator frees it stream-ordered)."""

    def __init__(self, cap: int = 4):
        self.cap = cap
        self.ws = {}

    def clear(self):
        self.ws = {}

    def get(self, key, nbytes_fn: Callable[[], int], dev: torch.device) -> torch.Tensor:
        ws = self.ws.pop(key, None)
        if ws is None:
            nbytes = int(nbytes_fn())
            while len(self.ws) >= self.cap:
                self.ws.pop(next(iter(self.ws)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.ws[key] = ws
        return ws


class NativeRuntime:
    """A native handle (``ghost_<prefix>_create`` .. ``_destroy``) with every packed tensor bound to its slot, for
    one (device, compute dtype); ``slots`` keeps the packed tensors alive.  ``what`` opens the error messages
    ("landmark ", or "" for the flagship)."""

    def __init__(self, prefix: str, what: str, dtype, slots, *create_args):
        self.lib = _lib.load()
        self.prefix, self.what, self.dtype = prefix, what, dtype
        self.h = None
        h = C.c_void_p()
        _lib.check(self._fn("create")(*create_args, C.byref(h)), f"ghost_{prefix}_create")
        self.h = h
        self.slots = slots
        self.ws = WorkspaceCache()   # key (ends in the stream) -> workspace (stream-ordered reuse)
        for name, t in slots.items():
            _lib.check(self._fn("bind")(h, name.encode(), t.data_ptr(), t.numel()), f"bind {name}")
        if self._fn("missing")(h) != 0:
            _lib.check(-2, f"{what}weights incomplete")

    def _fn(self, name: str):
        return getattr(self.lib, f"ghost_{self.prefix}_{name}")

    def workspace_for(self, nbytes_fn, key, dev: torch.device) -> torch.Tensor:
        """The cached workspace for ``key``, sized by ``nbytes_fn()`` (a negative size is the native error)."""

        def nbytes():
            n = nbytes_fn()
            if n < 0:
                _lib.check(int(n), f"{self.what}workspace sizing")
            return n
        return self.ws.get(key, nbytes, dev)

    def batch_workspace(self, N: int, dev: torch.device) -> torch.Tensor:
        """One workspace per (N, current stream of ``dev``), sized by ``ghost_<prefix>_workspace_bytes(h, N)``."""
        return self.workspace_for(lambda: self._fn("workspace_bytes")(self.h, N), (N, _lib.stream_ptr(dev)), dev)

    def _set_taps(self, ptrs):
        n = len(ptrs) if ptrs else 0
        return self._fn("set_taps")(self.h, (C.c_void_p * n)(*ptrs) if n else None, n)

    @contextlib.contextmanager
    def taps(self, ptrs, what: str):
        """Diagnostic tap pointers set for the calls inside the block and cleared after it, whatever happens."""
        _lib.check(self._set_taps(ptrs), what)
        try:
            yield
        finally:
            self._set_taps(None)

    def __del__(self):
        try:
            if self.h:
                self._fn("destroy")(self.h)
        except Exception:
            pass


def to_tensor(v) -> torch.Tensor:
    """A checkpoint value (torch tensor, numpy array or anything with ``.asnumpy()``) as a tensor of its own shape."""
    if torch.is_tensor(v):
        return v.detach()
    if hasattr(v, "asnumpy"):
        v = v.asnumpy()
    a = np.asarray(v)      # (np.ascontiguousarray would turn a 0-d array into [1])
    return torch.from_numpy(a if a.flags.c_contiguous else np.ascontiguousarray(a))


def load_named(own: dict, want: dict, given, model: str) -> None:
    """Copy ``given`` ({name: value}) into the tensors ``own``: exactly ``want``'s names ({name: shape}) and shapes."""
    missing = sorted(set(want) - set(given))
    extra = sorted(set(given) - set(want))
    if missing or extra:
        raise KeyError(f"ghost_amd: {model} parameters do not match: missing {missing}, unexpected {extra}")
    with torch.no_grad():
        for n, shape in want.items():
            t = to_tensor(given[n])
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"ghost_amd: {n} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            own[n].copy_(t.to(own[n].device, own[n].dtype))


def u8_rows(x: torch.Tensor, single_dense: bool = True):
    """uint8 [N,H,W,3] whose rows are contiguous, the batch possibly strided -> (tensor, batch stride in bytes),
    copying only when a sample itself is strided.  ``single_dense``: a batch of one is passed whole, with H*W*3
    as its stride."""
    H, W = x.shape[1], x.shape[2]
    if single_dense and x.shape[0] == 1:
        return (x if x.is_contiguous() else x.contiguous()), H * W * 3
    if x.shape[0] and x[0].stride() != (W * 3, 3, 1):
        x = x.contiguous()
    return x, x.stride(0)

"""bf16 weight shadows of the separate-parameter routes: one store of persistent bf16 slots per ``VisionTransformer3D``.

The GEMMs of the ``activations='bf16'`` routes (and of the bf16 inference forward) read their weights as bf16 through
``HipEncoder._bf16(name)``.  A slot is the persistent destination of that copy: made the first time a weight is asked for, shared by
the model's inference encoder and its trainer, dropped by ``set_precision``.  It records which state of the parameter it holds —
``p._version``, ``p.data_ptr()`` and the device — and is *current* only while all three still match; ``_bf16`` casts into a slot that
is not (``vitae_cast_bf16``), so whatever writes a weight (an optimiser of torch's, ``load_state_dict``, an in-place edit, ``.to()``)
costs one cast at the next forward, as it always did.

The three multi-tensor updaters (``MoCo._update_momentum_encoder``, ``LARS.step``, ``MultiTensorAdamW.norm_clip_step``) write the new
fp32 weight through raw pointers and bump its version.  They ask ``slot_for(p)``: a slot that is current at the time of the call is
listed in the launch's shadow column (``vitae_*_multi_shadow`` stores the bf16 copy in the same pass, 2 bytes per parameter) and marked
current at the new version afterwards; anything else is listed as 0 and left to the next forward's cast.  A stale slot is therefore
never validated by an update it did not see the input of, and a skipped AdamW step (nothing written, slot content still the
parameter's) stays correct.  ``VITAE_WEIGHT_SHADOW=0`` (read at call time) makes the updaters list nothing.

A slot hangs on its parameter object (no table keeps parameters alive, nothing compares tensors by value) and knows its owner by a
weak reference: a copied parameter that carries the attribute along is not the owner and gets a slot of its own.
"""
from __future__ import annotations

import os
import weakref
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

_ATTR = '_vitae_bf16_slot'


def enabled() -> bool:
    """Whether the updaters list shadows (``VITAE_WEIGHT_SHADOW``, default on; read at call time)."""
    return os.environ.get('VITAE_WEIGHT_SHADOW', '1') != '0'


class Slot:
    """The persistent bf16 copy of one parameter and the parameter state it was written from."""

    __slots__ = ('owner', 'data', 'version', 'ptr', 'device', '__weakref__')

    def __init__(self, p: torch.Tensor):
        self.owner = weakref.ref(p)
        self.data = torch.empty(p.numel(), dtype=torch.bfloat16, device=p.device)
        self.version, self.ptr, self.device = None, None, None

    def current(self) -> bool:
        p = self.owner()
        return p is not None and self.version == p._version and self.ptr == p.data_ptr() and self.device == p.device

    def mark(self):
        """The slot now holds the bf16 copy of its parameter as it is."""
        p = self.owner()
        self.version, self.ptr, self.device = p._version, p.data_ptr(), p.device

    def address(self) -> int:
        return self.data.data_ptr()

    def __reduce__(self):       # a pickled or deep-copied parameter / model carries no slot along: the copy makes its own
        return (_no_slot, ())


def _no_slot():
    return None


def slot_for(p: torch.Tensor) -> Optional[Slot]:
    """The slot of parameter ``p`` (None: it has none); ``.current()`` says whether it holds ``p`` as it is now."""
    s = getattr(p, _ATTR, None)
    return s if s is not None and s.owner() is p else None


class ShadowStore:
    """The slots of one model.  ``slot(p)`` makes the slot on first use (and again when the parameter moved to another device or
    changed its size); ``drop()`` detaches every slot from its parameter."""

    def __init__(self):
        self._slots: List[Slot] = []

    def slot(self, p: torch.Tensor) -> Slot:
        s = slot_for(p)
        if s is None or s.data.device != p.device or s.data.numel() != p.numel():
            if s in self._slots:
                self._slots.remove(s)
            s = Slot(p)
            setattr(p, _ATTR, s)
            self._slots.append(s)
        return s

    def slots(self) -> List[Slot]:
        return [s for s in self._slots if s.owner() is not None]

    def drop(self):
        for s in self._slots:
            p = s.owner()
            if p is not None and getattr(p, _ATTR, None) is s:
                delattr(p, _ATTR)
        self._slots = []

    def __reduce__(self):
        return (ShadowStore, ())


def store_of(module) -> ShadowStore:
    """The store of ``module`` (a ``VisionTransformer3D``), made on first use."""
    st = getattr(module, '_shadow', None)
    if st is None:
        st = ShadowStore()
        module._shadow = st
    return st


def shadow_column(params: Sequence[torch.Tensor]) -> Tuple[Optional[np.ndarray], List[Slot]]:
    """What an updater lists for ``params`` (the tensors of its table, in table order): (int64 addresses, 0 where the parameter has no
    slot or its slot is not current; the listed slots).  (None, []) when nothing is listed — the switch is off, or no slot is current —
    and the updater calls the entry point without a shadow column."""
    if not enabled():
        return None, []
    col = np.zeros(len(params), dtype=np.int64)
    listed: List[Slot] = []
    for t, p in enumerate(params):
        s = slot_for(p)
        if s is not None and s.current():
            col[t] = s.address()
            listed.append(s)
    return (col, listed) if listed else (None, [])


def mark_current(listed: Sequence[Slot]):
    """After the launch and ``increment_version``: the listed slots hold their parameters at the new version."""
    for s in listed:
        s.mark()


def pack_words(table: np.ndarray, hyper: Sequence[float] = (), shadow: Optional[np.ndarray] = None) -> np.ndarray:
    """The 64-bit words an updater sends in one copy, in front of the chunk list: [table entries | hyper-parameters (fp32, padded to a
    whole word) | shadow column].  The VITAE_MULTI_ENTRY_WORDS-word entries are the same with and without a shadow column; the
    column is one word per entry, in entry order."""
    parts = [np.ascontiguousarray(table, dtype=np.int64).reshape(-1)]
    if len(hyper):
        h = np.zeros(2 * ((len(hyper) + 1) // 2), dtype=np.float32)
        h[:len(hyper)] = hyper
        parts.append(h.view(np.int64))
    if shadow is not None:
        shadow = np.ascontiguousarray(shadow, dtype=np.int64).reshape(-1)
        if len(shadow) != len(table):
            raise ValueError('the shadow column has one address per table entry')
        parts.append(shadow)
    return np.concatenate(parts)

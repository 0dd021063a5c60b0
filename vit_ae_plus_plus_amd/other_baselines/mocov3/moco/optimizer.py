"""LARS of the MoCo v3 baseline (reference other_baselines/mocov3/moco/optimizer.py) as two HIP launches per step.

Same constructor, ``param_groups`` and per-parameter state (``{'mu'}``) as the reference's class, so state dicts interchange; ``step()``
is ``vitae_lars_multi`` over the tensor table that ``optim.MultiTensorAdamW`` introduced.  ``TableRing`` is that table's transport (a ring
of pinned slots, one host-to-device copy per call); ``builder.MoCo._update_momentum_encoder`` sends its table the same way.
"""
from __future__ import annotations

import numpy as np
import torch

from ...._abi import CONSTS, VitaeError, lib
from ....optim import multi_chunk_list
from ....shadow import mark_current, pack_words, shadow_column


class TableRing:
    """Sends [table | hyper-parameters (fp32) | chunk list (int32 pairs)] to the device for one multi-tensor launch group: a ring of
    pinned host slots ordered by events, one non-blocking copy on torch's current stream; the chunk list travels only when the slot does
    not hold the one of this set of lengths yet.  The host waits only when it is a whole ring of calls ahead of the device."""

    RING = 8

    def __init__(self):
        self._d = None

    def _buffers(self, device, words):
        d = self._d
        if d is None or d['device'] != device:
            d = self._d = {'device': device, 'words': 0, 'seq': 0, 'key': None}
        if words > d['words']:
            d['words'] = words = max(words, 2 * d['words'])
            d['pinned'] = [torch.empty(words, dtype=torch.int64, pin_memory=True) for _ in range(self.RING)]
            d['table'] = [torch.empty(words, dtype=torch.int64, device=device) for _ in range(self.RING)]
            d['events'] = [None] * self.RING
            d['keys'] = [None] * self.RING
        return d

    def send(self, device, table: np.ndarray, lengths, hyper=(), shadow=None):
        """table: int64 [n_tensors, VITAE_MULTI_ENTRY_WORDS]; hyper: floats sent behind it; shadow: int64 [n_tensors] bf16 addresses sent
        behind those (``shadow.shadow_column``; None: no column).  -> dict of the launchers' arguments (``th`` / ``td``: table on host /
        device, ``ch`` / ``cd``: chunk list, ``hd``: hyper-parameters on the device, ``sh`` / ``sd``: shadow column or None, ``nt``, ``nc``,
        ``chunk``) and ``slot`` for ``done()``.  Call with the device current; follow the launches with ``done(slot)``."""
        chunk = int(CONSTS['VITAE_MULTI_CHUNK'])
        nt, ew = table.shape
        front = pack_words(table, hyper, shadow)       # everything in front of the chunk list: one copy carries it all
        base = front.size
        key = (chunk, device, tuple(lengths))
        d = self._d
        if d is None or d['device'] != device or d['key'] != key:
            chunks = multi_chunk_list(lengths, chunk)
            d = self._buffers(device, base + nt + 64 + (chunks.size + 1) // 2)
            d['key'], d['chunks'] = key, chunks
        chunks = d['chunks']
        if base + (chunks.size + 1) // 2 > d['words']:     # more words in front than when the buffers were sized
            d = self._buffers(device, base + nt + 64 + (chunks.size + 1) // 2)
        slot = d['seq'] % self.RING
        d['seq'] += 1
        if d['events'][slot] is not None:
            d['events'][slot].synchronize()        # the call that last used this slot, RING calls ago, has finished reading it
        pinned, dev = d['pinned'][slot], d['table'][slot]
        host = pinned.numpy()
        host[:base] = front
        words = base
        if d['keys'][slot] != (key, base):
            host[base:].view(np.int32)[:chunks.size] = chunks.reshape(-1)
            words += (chunks.size + 1) // 2
            d['keys'][slot] = (key, base)
        dev[:words].copy_(pinned[:words], non_blocking=True)
        th, td = pinned.data_ptr(), dev.data_ptr()
        so = 8 * (base - nt)                       # the shadow column is the last nt words in front of the chunk list
        return {'th': th, 'td': td, 'nt': nt, 'ch': th + 8 * base, 'cd': td + 8 * base, 'nc': len(chunks), 'chunk': chunk,
                'hd': td + 8 * nt * ew, 'sh': None if shadow is None else th + so, 'sd': None if shadow is None else td + so,
                'slot': slot}

    def done(self, slot, stream):
        d = self._d
        ev = d['events'][slot] or torch.cuda.Event()
        ev.record(stream)
        d['events'][slot] = ev


def fp32_on_device(t, what):
    if not (t.is_cuda and t.dtype is torch.float32 and t.is_contiguous()) or t.is_sparse:
        raise VitaeError(f'{what} must be contiguous fp32 on a ROCm device (got {t.dtype} on {t.device}); there is no CPU fallback')


def ema_table(pm_ptrs, pb_ptrs, lengths):
    """The tensor table of ``vitae_ema_multi``: int64 [n, VITAE_MULTI_ENTRY_WORDS] = pm (written), pb (read), 0, 0, n, 0."""
    t = np.zeros((len(lengths), CONSTS['VITAE_MULTI_ENTRY_WORDS']), dtype=np.int64)
    t[:, 0], t[:, 1], t[:, 4] = pm_ptrs, pb_ptrs, lengths
    return t


def lars_table(p_ptrs, g_ptrs, mu_ptrs, scaled, lengths, groups):
    """The tensor table of ``vitae_lars_multi``: int64 [n, VITAE_MULTI_ENTRY_WORDS] = p, g, mu, flags, n, group."""
    t = np.empty((len(lengths), CONSTS['VITAE_MULTI_ENTRY_WORDS']), dtype=np.int64)
    flags = [CONSTS['VITAE_LARS_FLAG_SCALED'] if s else 0 for s in scaled]
    for col, vals in enumerate((p_ptrs, g_ptrs, mu_ptrs, flags, lengths, groups)):
        t[:, col] = vals
    return t


class LARS(torch.optim.Optimizer):
    """Layer-wise adaptive rate scaling with momentum; vectors and scalars (norm weights, biases) are neither decayed nor scaled.

    Per parameter with a gradient: for ``p.ndim > 1``, ``dp = g + weight_decay p`` scaled by ``q = trust_coefficient |p| / |dp|`` (1 when
    either norm is 0); else ``dp = g``.  Then ``mu <- momentum mu + dp`` and ``p <- p - lr mu``.  The norms are summed in double, in a fixed
    order.  Parameters, gradients and ``mu`` must be contiguous fp32 on one ROCm device at ``step()`` (VitaeError otherwise); constructing,
    saving and loading work anywhere.  A step copies one table to the device and never waits for it."""

    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient)
        super().__init__(params, defaults)
        self._ring = TableRing()
        self._ws = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ng = len(self.param_groups)
        if ng > CONSTS['VITAE_MULTI_MAX_GROUPS']:
            raise VitaeError(f"LARS serves at most {CONSTS['VITAE_MULTI_MAX_GROUPS']} groups")
        params, p_ptrs, g_ptrs, mu_ptrs, scaled, lengths, groups = [], [], [], [], [], [], []
        device = None
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                fp32_on_device(p, 'LARS.step(): a parameter')
                fp32_on_device(g, 'LARS.step(): a gradient')
                st = self.state[p]
                if 'mu' not in st:
                    st['mu'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                mu = st['mu']
                fp32_on_device(mu, "LARS.step(): the state 'mu'")
                if g.shape != p.shape or mu.shape != p.shape or g.device != p.device or mu.device != p.device:
                    raise VitaeError('LARS.step(): a gradient or a state tensor is not beside its parameter')
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise VitaeError('LARS: all parameters must be on one device')
                if p.numel() == 0:
                    continue
                params.append(p)
                p_ptrs.append(p.data_ptr()); g_ptrs.append(g.data_ptr()); mu_ptrs.append(mu.data_ptr())
                scaled.append(p.ndim > 1); lengths.append(p.numel()); groups.append(gi)
        if not params:
            return loss
        hyper = [float(g[k]) for k in ('lr', 'weight_decay', 'momentum', 'trust_coefficient') for g in self.param_groups]
        column, listed = shadow_column(params)      # bf16 slots that hold these parameters as they are now (shadow.py)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream()
            a = self._ring.send(device, lars_table(p_ptrs, g_ptrs, mu_ptrs, scaled, lengths, groups), lengths, hyper, column)
            if self._ws is None or self._ws.device != device or self._ws.numel() < 2 * a['nc']:
                self._ws = torch.empty(2 * a['nc'], dtype=torch.float64, device=device)
            if a['sh'] is None:
                lib.vitae_lars_multi(a['th'], a['td'], a['nt'], a['ch'], a['cd'], a['nc'], a['chunk'], a['hd'], ng, self._ws.data_ptr(),
                                     stream.cuda_stream)
            else:
                lib.vitae_lars_multi_shadow(a['th'], a['td'], a['nt'], a['ch'], a['cd'], a['nc'], a['chunk'], a['hd'], ng,
                                            self._ws.data_ptr(), a['sh'], a['sd'], stream.cuda_stream)
            self._ring.done(a['slot'], stream)
        # the kernels wrote through raw pointers: autograd and everything keyed on p._version must see it; the bf16 slots listed above
        # were written in the same pass and hold the new version
        torch.autograd.graph.increment_version(params)
        mark_current(listed)
        return loss

"""AdamW over the engine's flat arenas (one fused streaming kernel per weight-decay segment).

``FusedAdamW(model, ...)`` is what new code should construct.  ``adopt(optimizer, model)`` lets an
unchanged reference script keep its ``torch.optim.AdamW(optim_factory.add_weight_decay(model, wd),
lr=..., betas=(0.9, 0.95))`` (k_fold_training_scripts/k_fold_cross_valid_combined_brats.py:168-169):
the torch optimizer object stays the owner of the hyper-parameters and of a (view-backed)
``state_dict``, while ``step()`` runs ``vitae_adamw_step`` on the arena.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _abi
from ._abi import VitaeError, lib
from .shadow import mark_current, pack_words, shadow_column


class FusedAdamW:
    """torch.optim-like facade: ``param_groups`` (lr is read from group 0 every step, so
    ``lr_sched.adjust_learning_rate`` works), ``zero_grad``, ``step``, ``state_dict``."""

    def __init__(self, model, lr=1e-3, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-8):
        self.model = model
        decay, no_decay = [], []
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            (no_decay if (p.ndim <= 1 or n.endswith('.bias')) else decay).append(p)
        self.param_groups = [{'params': no_decay, 'weight_decay': 0.0, 'lr': lr, 'betas': betas, 'eps': eps},
                             {'params': decay, 'weight_decay': weight_decay, 'lr': lr, 'betas': betas, 'eps': eps}]
        self.defaults = dict(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
        self._pending_state = None

    @property
    def engine(self):
        eng = self.model.engine
        if eng is None:
            return None
        if eng.opt_state is None:
            g = self.param_groups
            eng.init_optimizer(weight_decay=g[1]['weight_decay'], betas=g[1]['betas'], eps=g[1]['eps'])
            if self._pending_state is not None:
                self._restore(eng, self._pending_state)
                self._pending_state = None
        return eng

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g['params']:
                p.grad = None

    @torch.no_grad()
    def step(self):
        eng = self.engine
        if eng is None:
            raise VitaeError('FusedAdamW.step() before any forward/backward on the GPU')
        eng.weight_decay = self.param_groups[1]['weight_decay']
        eng.betas, eng.eps = self.param_groups[1]['betas'], self.param_groups[1]['eps']
        eng.optimizer_hparams(lr=self.param_groups[0]['lr'])
        eng.grad_norm_and_step()

    # ---- checkpointing: flat arenas + step (engine layout is deterministic for a given model)
    def state_dict(self):
        eng = self.engine
        state = {'step': 0, 'exp_avg': None, 'exp_avg_sq': None}
        if eng is not None:
            # (the wire format is fp32 whatever the engine stores: bf16 moments of the bf16 precision mode are widened here, narrowed by _restore)
            state = {'step': eng.read_opt_step(), 'exp_avg': eng.opt_state['exp_avg'].detach().float().cpu(),
                     'exp_avg_sq': eng.opt_state['exp_avg_sq'].detach().float().cpu(),
                     'layout': {k: (o, list(s)) for k, (o, s) in eng.layout.items()}}
        groups = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]
        return {'fused_adamw': state, 'param_groups': groups}

    def _restore(self, eng, state):
        if state.get('exp_avg') is not None:
            eng.opt_state['exp_avg'].copy_(state['exp_avg'])
            eng.opt_state['exp_avg_sq'].copy_(state['exp_avg_sq'])
        eng.write_opt_step(int(state.get('step', 0)))

    def load_state_dict(self, sd):
        for g, s in zip(self.param_groups, sd.get('param_groups', [])):
            g.update(s)
        state = sd.get('fused_adamw')
        if state is None:
            raise VitaeError('not a FusedAdamW state dict')
        if self.model.engine is not None:
            self._restore(self.engine, state)
        else:
            self._pending_state = state


class _AdoptedAdamW:
    """Runs a foreign torch.optim.AdamW's step on the engine arenas (see module docstring)."""

    def __init__(self, optimizer: torch.optim.AdamW, model):
        self.optimizer, self.model = optimizer, model
        eng = model.engine
        ids_decay = {id(p) for n, p in model._trainable_named if not (p.ndim <= 1 or n.endswith('.bias'))}
        wd = None
        for g in optimizer.param_groups:
            if g.get('amsgrad') or g.get('maximize'):
                raise VitaeError('amsgrad / maximize are not supported by the fused AdamW')
            for p in g['params']:
                if (id(p) in ids_decay) != (g['weight_decay'] != 0.0) and g['weight_decay'] != 0.0:
                    raise VitaeError('optimizer groups do not follow the decay / no-decay split of the arena')
            if g['weight_decay'] != 0.0:
                wd = g['weight_decay']
        n_opt = sum(len(g['params']) for g in optimizer.param_groups)
        if n_opt != len(model._trainable):
            raise VitaeError('optimizer does not hold exactly the model parameters')
        g0 = optimizer.param_groups[0]
        eng.init_optimizer(weight_decay=wd or 0.0, betas=tuple(g0['betas']), eps=g0['eps'])
        # resume: import existing per-parameter state, then re-publish it as views of the arenas
        step = 0
        for n, p in model._trainable_named:
            st = optimizer.state.get(p)
            o, shp = eng.layout[n]
            k = p.numel()
            if st:
                eng.opt_state['exp_avg'][o:o + k].view(shp).copy_(st['exp_avg'])
                eng.opt_state['exp_avg_sq'][o:o + k].view(shp).copy_(st['exp_avg_sq'])
                step = max(step, int(st['step']))
            optimizer.state[p] = {'step': torch.tensor(float(step)),
                                  'exp_avg': eng.opt_state['exp_avg'][o:o + k].view(shp),
                                  'exp_avg_sq': eng.opt_state['exp_avg_sq'][o:o + k].view(shp)}
        eng.write_opt_step(step)
        self.engine = eng
        if not getattr(optimizer, '_vitae_hooked', False):
            optimizer.register_state_dict_pre_hook(lambda opt: opt._vitae_adopter._publish_step(opt))
            optimizer._vitae_hooked = True
        self._orig_step = optimizer.step
        optimizer.step = self.step
        optimizer.engine = eng

    def _publish_step(self, optimizer):
        step = self.engine.read_opt_step()
        for st in optimizer.state.values():
            st['step'] = torch.tensor(float(step))

    @torch.no_grad()
    def step(self, closure=None):
        g0 = self.optimizer.param_groups[0]
        eng = self.engine
        eng.betas, eng.eps = tuple(g0['betas']), g0['eps']
        eng.optimizer_hparams(lr=g0['lr'])
        eng.grad_norm_and_step()


def _adoptable_weight_decay(optimizer, model):
    """The single non-zero weight decay of a torch.optim.AdamW whose groups follow the arena's decay / no-decay split
    (timm add_weight_decay: no decay iff ndim <= 1 or name ends with '.bias'), or None when the optimiser cannot be
    re-routed without changing results."""
    ids_decay = {id(p) for n, p in model._trainable_named if not (p.ndim <= 1 or n.endswith('.bias'))}
    ids_all = {id(p) for p in model._trainable}
    wds, seen = set(), set()
    g0 = optimizer.param_groups[0]
    for g in optimizer.param_groups:
        if g.get('amsgrad') or g.get('maximize') or 'lr_scale' in g:
            return None
        if g['lr'] != g0['lr'] or tuple(g['betas']) != tuple(g0['betas']) or g['eps'] != g0['eps']:
            return None
        for p in g['params']:
            if id(p) not in ids_all or id(p) in seen:
                return None
            seen.add(id(p))
            if (id(p) in ids_decay) != (g['weight_decay'] != 0.0):
                return None         # e.g. a plain AdamW(model.parameters(), weight_decay=wd): biases in a decayed group
        if g['weight_decay'] != 0.0:
            wds.add(g['weight_decay'])
    if seen != ids_all or len(wds) > 1:
        return None
    return wds.pop() if wds else 0.0


def adopt(optimizer, model) -> Optional[object]:
    """Make ``optimizer.step()`` run on the HIP engine when that is possible without changing results:
    FusedAdamW is returned as is; a plain torch.optim.AdamW over exactly the model's parameters, grouped like
    timm's add_weight_decay, is re-routed in place (again, with its state migrated, when the model rebuilt its engine after
    ``set_precision()`` / ``.to()``); anything else is left alone (returns None: the caller keeps torch's own step)."""
    if isinstance(optimizer, FusedAdamW):
        return optimizer
    if model.engine is None:
        return None
    if getattr(optimizer, 'engine', None) is model.engine:
        return optimizer
    if type(optimizer) is torch.optim.AdamW and _adoptable_weight_decay(optimizer, model) is not None:
        if getattr(optimizer, 'engine', None) is not None:      # adopted for an engine that no longer exists
            # the per-parameter 'step' tensors are only refreshed by the state_dict pre-hook: publish the old engine's count
            # now, so that the new adopter resumes from it (else the bias corrections restart next to warmed-up moments)
            optimizer._vitae_adopter._publish_step(optimizer)
            optimizer.step = optimizer._vitae_adopter._orig_step
        optimizer._vitae_adopter = _AdoptedAdamW(optimizer, model)
        return optimizer
    return None


# ----------------------------------------------------------------------------- fine-tuning: separate parameters, layer-decay groups
def multi_chunk_list(lengths, chunk: Optional[int] = None):
    """The (tensor, chunk) pairs that ``vitae_grad_sqnorm_multi`` / ``vitae_adamw_multi`` walk: an int32 array [n_chunks, 2]; chunk k
    of tensor t is its elements [k * chunk, min(n_t, (k + 1) * chunk)).  Every element of every tensor is in exactly one pair, in
    tensor order; an empty tensor has none."""
    import numpy as np
    chunk = int(chunk or _abi.CONSTS['VITAE_MULTI_CHUNK'])
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if chunk <= 0 or chunk % 4 or (lengths < 0).any():
        raise VitaeError('multi_chunk_list: chunk must be a positive multiple of 4 and lengths non-negative')
    counts = (lengths + chunk - 1) // chunk
    tensor = np.repeat(np.arange(len(lengths), dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    k = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)
    return np.stack([tensor, k], axis=1).astype(np.int32)


def multi_table(p_ptrs, g_ptrs, m_ptrs, v_ptrs, lengths, groups):
    """The tensor table of the same two launchers: int64 [n_tensors, VITAE_MULTI_ENTRY_WORDS] = p, g, exp_avg, exp_avg_sq, n, group."""
    import numpy as np
    t = np.empty((len(lengths), _abi.CONSTS['VITAE_MULTI_ENTRY_WORDS']), dtype=np.int64)
    for col, vals in enumerate((p_ptrs, g_ptrs, m_ptrs, v_ptrs, lengths, groups)):
        t[:, col] = vals
    return t


class MultiTensorAdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` whose ``step()`` is two HIP launches over all parameters of all groups, whatever their number:
    ``vitae_grad_sqnorm_multi`` (global gradient norm, in double) and ``vitae_adamw_multi`` (clipping and the update, each tensor with its
    group's ``lr`` and ``weight_decay``).  Constructor, ``param_groups`` (extra keys such as ``lr_scale`` are kept), ``state``
    (``{'step', 'exp_avg', 'exp_avg_sq'}`` per parameter), ``state_dict`` / ``load_state_dict`` / ``zero_grad`` / ``add_param_group`` are
    torch's: checkpoints interchange with ``torch.optim.AdamW`` both ways.

    ``norm_clip_step(max_norm)`` returns the pre-clip global gradient norm (a 0-dim device tensor: what ``get_grad_norm_`` and
    ``clip_grad_norm_`` return) and steps; ``step()`` is the same without clipping.  Deviations from ``clip_grad_norm_`` followed by
    ``torch.optim.AdamW.step``:
      * a non-finite norm skips the update and the step count (GradScaler.step's inf check; torch would write NaN into the weights);
      * clipping scales the gradient as it is read: ``.grad`` is not rewritten;
      * there is ONE applied-step count, kept on the device (the host does not know whether a step was skipped): the per-parameter
        ``'step'`` entries are refreshed from it when a state dict is taken — the only place that synchronises — and loaded state
        whose steps differ is refused.
    Parameters must be contiguous fp32 on a ROCm device at ``step()`` (VitaeError otherwise: no CPU fallback); constructing, loading and
    saving work on CPU tensors.  A step issues one host-to-device copy (the tensor table, from a ring of pinned slots ordered by events)
    on torch's current stream and never waits for the device unless the host is a whole ring of steps ahead."""

    RING = 8

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or capturable or differentiable:
            raise VitaeError('MultiTensorAdamW: amsgrad / maximize / capturable / differentiable are not supported')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._dev = None              # device / pinned buffers, made by the first step
        self._host_step = None        # applied-step count to upload before the next launch (after a load)
        self._cache = {}              # parameter -> (p address, m address, v address, n, m, v, device) as last judged
        self._chunk = int(_abi.CONSTS['VITAE_MULTI_CHUNK'])
        self.register_state_dict_pre_hook(MultiTensorAdamW._publish_step)
        self.register_load_state_dict_post_hook(MultiTensorAdamW._adopt_loaded_steps)

    # ---- state: torch's layout, one step count
    @staticmethod
    def _common_step(state) -> Optional[int]:
        steps = {int(float(st['step'])) for st in state.values() if 'step' in st}
        if len(steps) > 1:
            raise VitaeError(f'MultiTensorAdamW keeps one step count; the state holds {sorted(steps)}')
        return steps.pop() if steps else None

    def _adopt_loaded_steps(self):
        step = self._common_step(self.state)
        self._host_step = 0 if step is None else step
        for st in self.state.values():      # (a fused torch optimiser keeps them on the device)
            if 'step' in st:
                st['step'] = torch.tensor(float(self._host_step), dtype=torch.float32)

    def _publish_step(self):
        if self._dev is None or self._host_step is not None:
            return                          # nothing stepped since construction / the last load: the entries are current
        step = float(self._dev['state'][_abi.CONSTS['VITAE_MULTI_STATE_STEP']].item())
        for st in self.state.values():
            if 'step' in st:
                st['step'] = torch.tensor(step, dtype=torch.float32)

    def applied_steps(self) -> int:
        """AdamW steps applied so far (synchronises)."""
        if self._dev is None or self._host_step is not None:
            return int(self._host_step or self._common_step(self.state) or 0)
        return int(self._dev['state'][_abi.CONSTS['VITAE_MULTI_STATE_STEP']].item())

    def skipped_steps(self) -> int:
        """Steps skipped because the gradient norm was not finite (synchronises)."""
        return 0 if self._dev is None else int(self._dev['state'][_abi.CONSTS['VITAE_MULTI_STATE_SKIPPED']].item())

    @classmethod
    def from_torch(cls, optimizer):
        """Take over the groups and the state of a plain ``torch.optim.AdamW`` (the tensors are shared, not copied).  None, with nothing
        changed, when it cannot be served: amsgrad / maximize / capturable / differentiable, groups with different betas or eps, or
        more than VITAE_MULTI_MAX_GROUPS groups."""
        if not isinstance(optimizer, torch.optim.AdamW) or not optimizer.param_groups:
            return None
        g0 = optimizer.param_groups[0]
        if len(optimizer.param_groups) > _abi.CONSTS['VITAE_MULTI_MAX_GROUPS']:
            return None
        for g in optimizer.param_groups:
            if g.get('amsgrad') or g.get('maximize') or g.get('capturable') or g.get('differentiable'):
                return None
            if tuple(g['betas']) != tuple(g0['betas']) or g['eps'] != g0['eps']:
                return None
        step = cls._common_step(optimizer.state)
        groups = []
        for g in optimizer.param_groups:
            g = dict(g)
            g['foreach'] = g['fused'] = None
            groups.append(g)
        new = cls(groups, lr=optimizer.defaults['lr'], betas=optimizer.defaults['betas'], eps=optimizer.defaults['eps'],
                  weight_decay=optimizer.defaults['weight_decay'])
        for p, st in optimizer.state.items():
            new.state[p] = dict(st)
        if step is not None:
            new._adopt_loaded_steps()
        return new

    # ---- the step
    def _buffers(self, device, words):
        d = self._dev
        if d is None or d['device'] != device:
            c = _abi.CONSTS
            d = self._dev = {'device': device, 'words': 0, 'seq': 0,
                             'state': torch.zeros(c['VITAE_MULTI_STATE_COUNT'], dtype=torch.float32, device=device),
                             'acc': torch.zeros(c['VITAE_ACC_COUNT'], dtype=torch.float64, device=device)}
            if self._host_step is None:
                self._host_step = self._common_step(self.state) or 0
        if words > d['words']:
            d['words'] = words = max(words, 2 * d['words'])
            d['pinned'] = [torch.empty(words, dtype=torch.int64, pin_memory=True) for _ in range(self.RING)]
            d['table'] = [torch.empty(words, dtype=torch.int64, device=device) for _ in range(self.RING)]
            d['events'] = [None] * self.RING
            d['keys'] = [None] * self.RING
        return d

    @torch.no_grad()
    def norm_clip_step(self, max_norm=None):
        import numpy as np
        c = _abi.CONSTS
        if len(self.param_groups) > c['VITAE_MULTI_MAX_GROUPS']:
            raise VitaeError(f"MultiTensorAdamW serves at most {c['VITAE_MULTI_MAX_GROUPS']} groups")
        g0 = self.param_groups[0]
        params, p_ptrs, g_ptrs, m_ptrs, v_ptrs, lengths, groups = [], [], [], [], [], [], []
        device, cache = None, self._cache
        bad = 'MultiTensorAdamW.step(): parameters and gradients must be contiguous fp32 on a ROCm device; there is no CPU fallback '
        for gi, group in enumerate(self.param_groups):
            if tuple(group['betas']) != tuple(g0['betas']) or group['eps'] != g0['eps']:
                raise VitaeError('MultiTensorAdamW: betas and eps are one set per step; the groups differ')
            if group.get('amsgrad') or group.get('maximize'):
                raise VitaeError('MultiTensorAdamW: amsgrad / maximize are not supported')
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if not (g.is_cuda and g.dtype is torch.float32 and g.is_contiguous()):      # a new tensor every iteration
                    raise VitaeError(bad + f'(got a {g.dtype} gradient on {g.device})')
                pp = p.data_ptr()
                st = self.state[p]
                known = cache.get(p)
                # what cannot change between two steps without one of these changing too is judged once, not 150 times per step
                if known is None or known[0] != pp or known[4] is not st.get('exp_avg') or known[5] is not st.get('exp_avg_sq'):
                    if not (p.is_cuda and p.dtype is torch.float32 and p.is_contiguous()) or p.is_sparse:
                        raise VitaeError(bad + f'(got a {p.dtype} parameter on {p.device})')
                    if 'exp_avg' not in st:
                        st['step'] = torch.tensor(0.0, dtype=torch.float32)
                        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    m, v = st['exp_avg'], st['exp_avg_sq']
                    for x in (m, v):
                        if not (x.is_cuda and x.dtype is torch.float32 and x.is_contiguous() and x.device == p.device and x.numel() == p.numel()):
                            raise VitaeError('MultiTensorAdamW.step(): optimizer state must be contiguous fp32 beside its parameter')
                    known = cache[p] = (pp, m.data_ptr(), v.data_ptr(), p.numel(), m, v, p.device)
                if g.device != known[6] or g.numel() != known[3]:
                    raise VitaeError(bad + '(a gradient is not beside its parameter)')
                if device is None:
                    device = known[6]
                elif known[6] != device:
                    raise VitaeError('MultiTensorAdamW: all parameters must be on one device')
                if known[3] == 0:
                    continue
                params.append(p)
                p_ptrs.append(pp); g_ptrs.append(g.data_ptr()); m_ptrs.append(known[1]); v_ptrs.append(known[2])
                lengths.append(known[3]); groups.append(gi)
        if not params:
            dev = device or (self._dev['device'] if self._dev else g0['params'][0].device)
            return torch.zeros((), dtype=torch.float32, device=dev)
        nt, ew, ng = len(params), c['VITAE_MULTI_ENTRY_WORDS'], len(self.param_groups)
        key = (self._chunk, ng, device, tuple(lengths))
        d = self._dev
        if d is None or d.get('key') != key:
            chunks = multi_chunk_list(lengths, self._chunk)
            d = self._buffers(device, nt * ew + ng + nt + (chunks.size + 1) // 2)       # (room for a shadow column)
            d['key'], d['chunks'] = key, chunks
        d = self._buffers(device, 0)
        chunks = d['chunks']
        slot = d['seq'] % self.RING
        d['seq'] += 1
        if d['events'][slot] is not None:
            d['events'][slot].synchronize()      # the step that last used this slot, RING steps ago, has finished reading it
        pinned, table = d['pinned'][slot], d['table'][slot]
        host = pinned.numpy()
        # bf16 slots that hold these parameters as they are now get the new weights in the same pass (shadow.py); a slot that is stale
        # (a load_state_dict since the last forward, ...) is not listed, so this step cannot validate it
        column, listed = shadow_column(params)
        # [table | lr of every group, wd of every group (fp32) | shadow column, if any | chunk list (int32 pairs)], in 64-bit words
        hyper = [float(g['lr']) for g in self.param_groups] + [float(g['weight_decay']) for g in self.param_groups]
        front = pack_words(multi_table(p_ptrs, g_ptrs, m_ptrs, v_ptrs, lengths, groups), hyper, column)
        words = base = front.size
        host[:base] = front
        if d['keys'][slot] != (key, base):       # the chunk list travels with the table only when this slot does not hold it yet
            host[base:].view(np.int32)[:chunks.size] = chunks.reshape(-1)
            words += (chunks.size + 1) // 2
            d['keys'][slot] = (key, base)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream()
            table[:words].copy_(pinned[:words], non_blocking=True)
            if self._host_step is not None:      # after construction or a load: a one-off upload, not part of a steady step
                d['state'][c['VITAE_MULTI_STATE_STEP']] = float(self._host_step)
                self._host_step = None
            norm = torch.empty((), dtype=torch.float32, device=device)
            th, td = pinned.data_ptr(), table.data_ptr()
            lrd = td + 8 * nt * ew
            ch, cd = th + 8 * base, td + 8 * base
            lib.vitae_grad_sqnorm_multi(th, td, nt, ch, cd, len(chunks), self._chunk, d['acc'].data_ptr(), stream.cuda_stream)
            args = (th, td, nt, ch, cd, len(chunks), self._chunk, lrd, lrd + 4 * ng, ng,
                    float(g0['betas'][0]), float(g0['betas'][1]), float(g0['eps']),
                    float(max_norm) if max_norm is not None else 0.0, d['state'].data_ptr(), d['acc'].data_ptr(), norm.data_ptr())
            if column is None:
                lib.vitae_adamw_multi(*args, stream.cuda_stream)
            else:                                # the column is the last nt words in front of the chunk list
                lib.vitae_adamw_multi_shadow(*args, th + 8 * (base - nt), td + 8 * (base - nt), stream.cuda_stream)
            ev = d['events'][slot] or torch.cuda.Event()
            ev.record(stream)
            d['events'][slot] = ev
        # the kernels wrote through raw pointers: autograd (and everything keyed on p._version, the bf16 slots of shadow.py) must see it
        torch.autograd.graph.increment_version(params)
        # a skipped step wrote neither the weights nor the slots: the listed slots hold the (unchanged) weights at the new version too
        mark_current(listed)
        return norm

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.norm_clip_step(None)
        return loss

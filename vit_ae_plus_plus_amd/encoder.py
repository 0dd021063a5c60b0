"""Encoder-only inference on MI355X: the kernel sequence behind ``VisionTransformer3D.forward_features``
(reference model/vit.py:265-284, driven by utils/feature_extraction.py:9-45 after pre-training).

Same kernels as the training engine's encoder, unmasked (every patch is kept, N = L + 1 tokens):
patch gather -> patch-embedding GEMM -> cls/pos assembly -> depth x [LN, qkv, attention, proj(+res), LN,
fc1+GELU, fc2(+res)] -> global-pool mean + fc_norm, or norm of the cls rows.  Nothing is kept for a
backward pass, so two activation buffers ping-pong through the blocks.

bf16 mode (the counterpart of the reference's ``torch.cuda.amp.autocast()`` around forward_features)
keeps GEMM operands in bf16 written by their producers and runs every Linear on the LDS-DMA GEMM when
all contraction lengths are multiples of 64; otherwise, and in fp32 mode, the generic Linear launcher
(exact-fp32 MFMA or bf16 MFMA with fp32 activations) is used.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from ._abi import CONSTS as _C, VitaeError, lib

PREC = {'fp32': _C['VITAE_PREC_F32'], 'bf16': _C['VITAE_PREC_BF16'], 'fp32x3': _C['VITAE_PREC_BF16X3']}
EPI_NONE, EPI_GELU = _C['VITAE_EPI_NONE'], _C['VITAE_EPI_GELU']


def _ptr(t):
    return None if t is None else t.data_ptr()


class HipEncoder:
    """Sequences the encoder kernels for one ``VisionTransformer3D`` instance (weights are read from the
    module's parameters at call time; bf16 copies are cached per parameter version)."""

    def __init__(self, module, precision: str = 'fp32'):
        if precision not in PREC:
            raise VitaeError(f'unknown precision {precision!r}')
        lib.load()
        self.m = module
        self.precision, self.prec = precision, PREC[precision]
        self._w16: Dict[str, Tuple[int, torch.Tensor]] = {}
        self._B = None
        self.buf: Dict[str, torch.Tensor] = {}
        self._split: Dict[Tuple, int] = {}

    # ------------------------------------------------------------------ parameters
    def _param(self, name: str):
        p = self.sd.get(name)
        if p is None:        # e.g. qkv_bias=False
            return None
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
            raise VitaeError(f'parameter {name} must be contiguous fp32 on {self.device}')
        return p

    def _bf16(self, name: str) -> int:
        p = self._param(name)
        ent = self._w16.get(name)
        if ent is None or ent[0] != p._version or ent[1].device != p.device:
            t = torch.empty(p.numel(), dtype=torch.bfloat16, device=p.device)
            lib.vitae_cast_bf16(p.data_ptr(), t.data_ptr(), p.numel(), self.stream)
            ent = (p._version, t)
            self._w16[name] = ent
        return ent[1].data_ptr()

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int):
        m = self.m
        L, D, H, P = m.patch_embed.num_patches, m.embed_dim, self.hidden, self.P
        N = L + 1
        M = B * N
        if self._B == (B, self.device):
            return
        self._B = (B, self.device)
        dev = self.device
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b = self.buf = {}
        b['ids'] = torch.arange(L, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
        b['tok'] = f(B * L, D)
        b['xa'], b['xb'], b['xmid'] = f(M, D), f(M, D), f(M, D)
        b['qkv'], b['o'], b['lse'] = f(M, 3 * D), f(M, D), f(B * m.num_heads * N)
        b['mean'], b['rstd'] = f(max(M, B)), f(max(M, B))
        b['hpre'] = f(M, H)
        b['pool'], b['feat'] = f(B, D), f(B, D)
        if self.act16:
            z16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
            b['patches_16'] = z16(B * L, P)
            b['y_16'], b['o_16'], b['act_16'] = z16(M, D), z16(M, D), z16(M, H)
            b['ws16'] = torch.zeros(1 << 22, dtype=torch.float32, device=dev)
        else:
            b['patches'], b['y'], b['act'] = f(B * L, P), f(M, D), f(M, H)
            b['ws'] = f(1 << 22)

    # ------------------------------------------------------------------ launch helpers
    def _g16(self, x16, wname, bname, M, N, K, y=None, y16=None, epi=EPI_NONE, aux=None, res=None):
        key = ('g', M, N, K, epi)
        s = self._split.get(key)
        if s is None:
            s = 1 if (epi & 15) == EPI_GELU else lib.vitae_gemm_glds_pick_split_k(M, N, K)     # (flags are OR-ed in above bit 3)
            while s > 1 and lib.vitae_gemm_glds_ws_floats(M, N, s) > self.buf['ws16'].numel():
                s -= 1
            self._split[key] = s
        lib.vitae_gemm_glds(1, 1, _ptr(x16), K, self._bf16(wname), K, _ptr(y), N, _ptr(y16), N, M, N, K,
                            _ptr(self._param(bname)), _ptr(res), N, epi, _ptr(aux), N, 0, s, self.buf['ws16'].data_ptr(), None,
                            self.stream)

    def _lin(self, x, wname, bname, y, M, N, K, epi=EPI_NONE, aux=None, res=None):
        key = ('l', M, N, K, epi)
        s = self._split.get(key)
        if s is None:
            s = 1 if epi != EPI_NONE else lib.vitae_gemm_pick_split_k(M, N, K)
            while s > 1 and s * M * N > self.buf['ws'].numel():
                s -= 1
            self._split[key] = s
        lib.vitae_linear_fwd(self.prec, _ptr(x), _ptr(self._param(wname)), _ptr(self._param(bname)), _ptr(y), M, N, K, epi,
                             _ptr(aux), _ptr(res), s, self.buf['ws'].data_ptr(), self.stream)

    def _ln(self, x, pre, y, y16, M, D):
        b = self.buf
        lib.vitae_layernorm_fwd(_ptr(x), _ptr(self._param(pre + 'weight')), _ptr(self._param(pre + 'bias')), _ptr(y), _ptr(y16),
                                _ptr(b['mean']), _ptr(b['rstd']), M, D, self.eps, self.stream)

    def _sdpa(self, B, N):
        b, m = self.buf, self.m
        if self.prec == PREC['bf16'] and self.hd in (32, 64):
            lib.vitae_sdpa_mfma_fwd(_ptr(b['qkv']), _ptr(b['o']), _ptr(b['o_16']) if self.act16 else None, _ptr(b['lse']), B, N,
                                    m.num_heads, self.hd, self.stream)
        else:
            lib.vitae_sdpa_fwd(_ptr(b['qkv']), _ptr(b['o']), _ptr(b['lse']), B, N, m.num_heads, self.hd, self.stream)

    # ------------------------------------------------------------------ forward
    def _begin(self, x: torch.Tensor):
        """Checks the input against the module and fixes the geometry of this call (device, stream, parameter table, sizes)."""
        m = self.m
        if not x.is_cuda:
            raise VitaeError(f'forward_features: input is on {x.device}; this package computes on MI355X only (no CPU fallback)')
        self.device = x.device
        self.stream = torch.cuda.current_stream(x.device).cuda_stream
        self.sd = dict(m.named_parameters())
        pe = m.patch_embed
        ps = pe.patch_size[0]
        if pe.patch_size != (ps, ps, ps) or ps % 4:
            raise VitaeError('patch_size must be cubic and a multiple of 4')
        B, C, Lz, Hy, Wx = x.shape
        assert (Lz, Hy, Wx) == tuple(pe.volume_size), \
            f"Volume image size ({Lz}*{Hy}*{Wx}) doesn't match model ({pe.volume_size[0]}*{pe.volume_size[1]}*{pe.volume_size[2]})."
        self.P = C * ps ** 3
        self.hidden = m.blocks[0].mlp.fc1.out_features if len(m.blocks) else m.embed_dim
        self.hd = m.embed_dim // m.num_heads
        self.eps = m.ln_eps
        return B, C, Lz, Hy, Wx, ps

    @torch.no_grad()
    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        m = self.m
        B, C, Lz, Hy, Wx, ps = self._begin(x)
        L, D = m.patch_embed.num_patches, m.embed_dim
        N, M = L + 1, B * (L + 1)
        H, P = self.hidden, self.P
        self.act16 = (self.prec == PREC['bf16'] and all(v % 64 == 0 for v in (D, H, P)) and self.hd in (32, 64))
        self._alloc(B)
        b, st = self.buf, self.stream
        xc = x.contiguous().float()
        a16 = self.act16
        lib.vitae_gather_patches(_ptr(xc), _ptr(b['ids']), None if a16 else _ptr(b['patches']), _ptr(b['patches_16']) if a16 else None,
                                 B, C, Lz, Hy, Wx, ps, L, st)
        if a16:
            self._g16(b['patches_16'], 'patch_embed.proj.weight', 'patch_embed.proj.bias', B * L, D, P, y=b['tok'])
        else:
            self._lin(b['patches'], 'patch_embed.proj.weight', 'patch_embed.proj.bias', b['tok'], B * L, D, P)
        lib.vitae_encoder_assemble_fwd(_ptr(b['tok']), _ptr(self._param('cls_token')), _ptr(self._param('pos_embed')),
                                       _ptr(b['ids']), _ptr(b['xa']), B, L, L, D, st)
        cur, nxt = b['xa'], b['xb']
        for i in range(len(m.blocks)):
            q = f'blocks.{i}.'
            if a16:
                self._ln(cur, q + 'norm1.', None, b['y_16'], M, D)
                self._g16(b['y_16'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', M, 3 * D, D, y=b['qkv'])
                self._sdpa(B, N)
                self._g16(b['o_16'], q + 'attn.proj.weight', q + 'attn.proj.bias', M, D, D, y=b['xmid'], res=cur)
                self._ln(b['xmid'], q + 'norm2.', None, b['y_16'], M, D)
                self._g16(b['y_16'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', M, H, D, y16=b['act_16'], epi=EPI_GELU, aux=b['hpre'])
                self._g16(b['act_16'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', M, D, H, y=nxt, res=b['xmid'])
            else:
                self._ln(cur, q + 'norm1.', b['y'], None, M, D)
                self._lin(b['y'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', b['qkv'], M, 3 * D, D)
                self._sdpa(B, N)
                self._lin(b['o'], q + 'attn.proj.weight', q + 'attn.proj.bias', b['xmid'], M, D, D, res=cur)
                self._ln(b['xmid'], q + 'norm2.', b['y'], None, M, D)
                self._lin(b['y'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', b['act'], M, H, D, epi=EPI_GELU, aux=b['hpre'])
                self._lin(b['act'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', nxt, M, D, H, res=b['xmid'])
            cur, nxt = nxt, cur
        if m.global_pool:
            lib.vitae_mean_pool_tokens(_ptr(cur), _ptr(b['pool']), B, N, D, 1, st)
            self._ln(b['pool'], 'fc_norm.', b['feat'], None, B, D)
        else:
            # LayerNorm is row-wise: normalising only the cls rows equals norm(x)[:, 0] (model/vit.py:281-282)
            b['pool'].copy_(cur.view(B, N, D)[:, 0])
            self._ln(b['pool'], 'norm.', b['feat'], None, B, D)
        return b['feat'].clone()


EPI_DGELU, EPI_AUX_DERIV = _C['VITAE_EPI_DGELU'], _C['VITAE_EPI_AUX_DERIV']
_EMBED = ('cls_token', 'pos_embed', 'patch_embed.proj.weight', 'patch_embed.proj.bias')


class HipEncoderTrainer(HipEncoder):
    """Training counterpart of ``HipEncoder`` (fine-tuning, reference post_training_utils/fine_tune_epoch.py:34-100):
    ``forward_keep`` runs the same launch sequence on the generic Linear launchers and keeps, per block, what the backward
    reads; ``backward`` walks the blocks from the top in the launch order of ``HipMAEEngine._block_bwd`` — eager launches
    on the current stream, no side streams, no graph capture.

    The kept activations are allocated per call and returned to the caller (who hangs them on the autograd context), so any
    number of forwards may precede a backward.  Only split-K scratch and the patch index table live on the trainer.
    Gradients are produced for the parameters named in ``needs`` only: a frozen Linear has no weight-gradient launch, and
    blocks below the lowest trainable parameter are neither kept nor walked.  ``stats`` counts the calls and the bytes the
    last forward kept (tests read it; nothing else does)."""

    WS_FLOATS = 1 << 24        # split-K scratch, 64 MiB (as the training engine's)

    def __init__(self, module, precision: str = 'fp32'):
        super().__init__(module, precision)
        self.act16 = False     # fp32 activations on the generic launchers; HipEncoderTrainer16 is the bf16-activation route
        self.stats = {'forwards': 0, 'backwards': 0, 'kept_bytes': 0, 'route': 'fp32-activations'}

    def _workspace(self, B: int, L: int):
        if self._B != self.device:          # scratch does not depend on the batch: forwards of different sizes may interleave
            self._B = self.device
            self.buf = {'ws': torch.empty(self.WS_FLOATS, dtype=torch.float32, device=self.device)}
        if ('ids', B) not in self.buf:
            self.buf['ids', B] = torch.arange(L, dtype=torch.int32, device=self.device).repeat(B, 1).contiguous()
        return self.buf['ids', B]

    def _f(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _z(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.device)

    @staticmethod
    def lowest_trainable(needs: Dict[str, bool], depth: int) -> Tuple[bool, int]:
        """(an embedding parameter is trainable, index of the lowest block the backward has to reach: ``depth`` = none)."""
        embed = any(needs.get(n, False) for n in _EMBED)
        if embed:
            return True, 0
        lo = depth
        for n, need in needs.items():
            if need and n.startswith('blocks.'):
                lo = min(lo, int(n.split('.')[1]))
        return False, lo

    # ------------------------------------------------------------------ forward
    def _ln_keep(self, x, pre, y, mean, rstd, M, D):
        lib.vitae_layernorm_fwd(_ptr(x), _ptr(self._param(pre + 'weight')), _ptr(self._param(pre + 'bias')), _ptr(y), None,
                                _ptr(mean), _ptr(rstd), M, D, self.eps, self.stream)

    def _block_keep(self, q, x_in, B, N, D, H):
        f, M, heads = self._f, B * N, self.m.num_heads
        k = {'x_in': x_in, 'mean1': f(M), 'rstd1': f(M), 'y1': f(M, D), 'qkv': f(M, 3 * D), 'o': f(M, D), 'lse': f(B * heads * N),
             'xmid': f(M, D), 'mean2': f(M), 'rstd2': f(M), 'y2': f(M, D), 'hpre': f(M, H), 'act': f(M, H)}
        x_out = f(M, D)
        self._ln_keep(x_in, q + 'norm1.', k['y1'], k['mean1'], k['rstd1'], M, D)
        self._lin(k['y1'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', k['qkv'], M, 3 * D, D)
        if self.prec == PREC['bf16'] and self.hd in (32, 64):
            lib.vitae_sdpa_mfma_fwd(_ptr(k['qkv']), _ptr(k['o']), None, _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        else:
            lib.vitae_sdpa_fwd(_ptr(k['qkv']), _ptr(k['o']), _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        self._lin(k['o'], q + 'attn.proj.weight', q + 'attn.proj.bias', k['xmid'], M, D, D, res=x_in)
        self._ln_keep(k['xmid'], q + 'norm2.', k['y2'], k['mean2'], k['rstd2'], M, D)
        # aux <- GELU'(pre-activation): what the backward multiplies by (as the training engine keeps it)
        self._lin(k['y2'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', k['act'], M, H, D, epi=EPI_GELU | EPI_AUX_DERIV, aux=k['hpre'])
        self._lin(k['act'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', x_out, M, D, H, res=k['xmid'])
        return k, x_out

    def forward_keep(self, x: torch.Tensor, needs: Dict[str, bool]):
        """-> (features [B, D], kept): ``kept`` is what ``backward`` needs, owned by the caller."""
        m = self.m
        B, C, Lz, Hy, Wx, ps = self._begin(x)
        L, D, H, P = m.patch_embed.num_patches, m.embed_dim, self.hidden, self.P
        N, M, depth = L + 1, B * (L + 1), len(m.blocks)
        if D % 4:
            raise VitaeError('embed_dim must be a multiple of 4')
        ids = self._workspace(B, L)
        f, st = self._f, self.stream
        embed, lo = self.lowest_trainable(needs, depth)
        xc = x.detach().contiguous().float()
        patches, tok, cur = f(B * L, P), f(B * L, D), f(M, D)
        lib.vitae_gather_patches(_ptr(xc), _ptr(ids), _ptr(patches), None, B, C, Lz, Hy, Wx, ps, L, st)
        self._lin(patches, 'patch_embed.proj.weight', 'patch_embed.proj.bias', tok, B * L, D, P)
        lib.vitae_encoder_assemble_fwd(_ptr(tok), _ptr(self._param('cls_token')), _ptr(self._param('pos_embed')), _ptr(ids),
                                       _ptr(cur), B, L, L, D, st)
        blocks = {}
        for i in range(depth):
            kb, cur = self._block_keep(f'blocks.{i}.', cur, B, N, D, H)
            if i >= lo:
                blocks[i] = kb
        pool, feat, mean, rstd = f(B, D), f(B, D), f(B), f(B)
        if m.global_pool:
            lib.vitae_mean_pool_tokens(_ptr(cur), _ptr(pool), B, N, D, 1, st)
            self._ln_keep(pool, 'fc_norm.', feat, mean, rstd, B, D)
        else:
            pool.copy_(cur.view(B, N, D)[:, 0])
            self._ln_keep(pool, 'norm.', feat, mean, rstd, B, D)
        kept = {'geom': (B, L, D, H, P), 'needs': dict(needs), 'params': self.sd, 'embed': embed, 'lo': lo, 'blocks': blocks,
                'versions': {n: p._version for n, p in self.sd.items() if not n.startswith('head.')},
                'patches': patches if needs.get('patch_embed.proj.weight') else None, 'pool': pool, 'mean': mean, 'rstd': rstd}
        self.stats['forwards'] += 1
        self.stats['kept_bytes'] = 4 * (sum(t.numel() for kb in blocks.values() for t in kb.values())
                                        + sum(t.numel() for t in (kept['patches'], pool, mean, rstd) if t is not None))
        return feat, kept

    # ------------------------------------------------------------------ backward
    def _split_bwd(self, M, N, K):
        """Split of the reduction (length K) of a backward GEMM with an [M, N] result, fitted to the scratch buffer."""
        key = ('b', M, N, K)
        s = self._split.get(key)
        if s is None:
            s = (lib.vitae_gemm_bf16x3_pick_split_k if self.prec == PREC['fp32x3'] else lib.vitae_gemm_pick_split_k)(M, N, K)
            while s > 1 and s * M * N > self.buf['ws'].numel():
                s -= 1
            self._split[key] = s
        return s

    def _lin_bwd(self, grads, needs, dy, wname, bname, x, dx, M, N, K, epi=EPI_NONE, aux=None):
        """Backward of y = x W^T + b given dy [M, N]: dW = dy^T x and db = colsum(dy) for trainable parameters only,
        dx = epi(dy W) when ``dx`` is given."""
        ws = self.buf['ws'].data_ptr()
        if needs.get(wname):
            w = self._param(wname)
            dw = grads[wname] = torch.empty_like(w)
            lib.vitae_linear_bwd_weight(self.prec, _ptr(dy), _ptr(x), _ptr(dw), M, N, K, 0, self._split_bwd(N, K, M), ws, self.stream)
        if needs.get(bname):
            db = grads[bname] = self._z(N)          # the column-sum launcher adds
            lib.vitae_colsum_accum(_ptr(dy), N, _ptr(db), M, N, self.stream)
        if dx is not None:
            lib.vitae_linear_bwd_input(self.prec, _ptr(dy), _ptr(self._param(wname)), _ptr(dx), M, N, K, epi, _ptr(aux), 0,
                                       self._split_bwd(M, K, N), ws, self.stream)

    def _ln_bwd(self, grads, needs, dy, x, pre, mean, rstd, dx, M, D, dx_accumulate):
        dw, db = self._z(D), self._z(D)             # the launcher adds its column partials
        lib.vitae_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(self._param(pre + 'weight')), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dw),
                                _ptr(db), None, None, M, D, dx_accumulate, self.stream)
        if needs.get(pre + 'weight'):
            grads[pre + 'weight'] = dw
        if needs.get(pre + 'bias'):
            grads[pre + 'bias'] = db

    def backward(self, kept, dfeat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """d loss / d features [B, D] -> {parameter name: gradient} for the trainable parameters of the encoder."""
        m = self.m
        B, L, D, H, P = kept['geom']
        N, M, depth, heads = L + 1, B * (L + 1), len(m.blocks), m.num_heads
        self.device = dfeat.device
        self.stream = torch.cuda.current_stream(dfeat.device).cuda_stream
        self.sd = kept['params']
        stale = [n for n, v in kept['versions'].items() if self.sd[n]._version != v]
        if stale:       # the backward reads the weights again: they must be the ones the forward used (as autograd checks for its own ops)
            raise VitaeError(f'parameters were modified in place between forward and backward: {stale[:3]} ...')
        self._workspace(B, L)
        needs, f, st = kept['needs'], self._f, self.stream
        grads: Dict[str, torch.Tensor] = {}
        dfeat = dfeat.contiguous().float()
        dpool = f(B, D)
        self._ln_bwd(grads, needs, dfeat, kept['pool'], 'fc_norm.' if m.global_pool else 'norm.', kept['mean'], kept['rstd'],
                     dpool, B, D, 0)
        self.stats['backwards'] += 1
        embed, lo = kept['embed'], kept['lo']
        if not embed and lo >= depth:
            return grads
        dx = f(M, D)
        lib.vitae_token_select_bwd(_ptr(dpool), _ptr(dx), B, N, D, 1 if m.global_pool else 0, st)
        dh, dy, do, dqkv, delta = f(M, H), f(M, D), f(M, D), f(M, 3 * D), f(B * heads * N)
        mfma = self.prec == PREC['bf16'] and self.hd in (32, 64)
        for i in range(depth - 1, lo - 1, -1):
            q, k = f'blocks.{i}.', kept['blocks'][i]
            self._lin_bwd(grads, needs, dx, q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', k['act'], dh, M, D, H,
                          epi=EPI_DGELU | EPI_AUX_DERIV, aux=k['hpre'])
            self._lin_bwd(grads, needs, dh, q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', k['y2'], dy, M, H, D)
            self._ln_bwd(grads, needs, dy, k['xmid'], q + 'norm2.', k['mean2'], k['rstd2'], dx, M, D, 1)
            self._lin_bwd(grads, needs, dx, q + 'attn.proj.weight', q + 'attn.proj.bias', k['o'], do, M, D, D)
            if mfma:
                lib.vitae_sdpa_mfma_bwd(_ptr(k['qkv']), _ptr(k['o']), _ptr(do), _ptr(k['lse']), _ptr(dqkv), None, None, _ptr(delta),
                                        B, N, heads, self.hd, st)
            else:
                lib.vitae_sdpa_bwd(_ptr(k['qkv']), _ptr(k['o']), _ptr(do), _ptr(k['lse']), _ptr(dqkv), _ptr(delta), B, N, heads,
                                   self.hd, st)
            self._lin_bwd(grads, needs, dqkv, q + 'attn.qkv.weight', q + 'attn.qkv.bias', k['y1'], dy, M, 3 * D, D)
            self._ln_bwd(grads, needs, dy, k['x_in'], q + 'norm1.', k['mean1'], k['rstd1'], dx, M, D, 1)
        if embed:
            patch = needs.get('patch_embed.proj.weight') or needs.get('patch_embed.proj.bias')
            dtok = f(B * L, D) if patch else None
            dpos = grads['pos_embed'] = torch.empty_like(self._param('pos_embed')) if needs.get('pos_embed') else None
            dcls = grads['cls_token'] = torch.empty_like(self._param('cls_token')) if needs.get('cls_token') else None
            lib.vitae_vit_assemble_bwd(_ptr(dx), _ptr(dtok), None, _ptr(dpos), _ptr(dcls), B, L, D, 0, st)
            if patch:
                self._lin_bwd(grads, needs, dtok, 'patch_embed.proj.weight', 'patch_embed.proj.bias', kept['patches'], None,
                              B * L, D, P)
        return {n: g for n, g in grads.items() if g is not None}


EPI_AUX_BF16 = _C['VITAE_EPI_AUX_BF16']


def act16_refusal(precision, embed_dim, hidden, patch_dim, head_dim):
    """Why the bf16-activation route does not serve this model (None: it does) — the rule ``HipEncoder.forward_features`` applies
    to ``act16``: bf16 arithmetic, every contraction length a multiple of the LDS-DMA GEMM's 64-wide k-tile, an MFMA head size."""
    if precision != 'bf16':
        return f"activations='bf16' needs precision='bf16' (got {precision!r})"
    bad = {k: v for k, v in (('embed_dim', embed_dim), ('MLP hidden size', hidden), ('in_chans * patch_size^3', patch_dim)) if v % 64}
    if bad:
        return f"activations='bf16' needs multiples of 64, got {bad}"
    if head_dim not in (32, 64):
        return f"activations='bf16' needs a head size of 32 or 64 (got {head_dim})"
    return None


def act16_refusal_for(module, precision, in_chans=None):
    """``act16_refusal`` for a ``VisionTransformer3D`` (``in_chans``: of the input at hand; default: of the patch embedding)."""
    pe = module.patch_embed
    hidden = module.blocks[0].mlp.fc1.out_features if len(module.blocks) else module.embed_dim
    c = pe.proj.in_channels if in_chans is None else in_chans
    return act16_refusal(precision, module.embed_dim, hidden, c * pe.patch_size[0] * pe.patch_size[1] * pe.patch_size[2],
                         module.embed_dim // module.num_heads)


class HipEncoderTrainer16(HipEncoderTrainer):
    """The bf16-activation training route (``VisionTransformer3D(precision='bf16', activations='bf16')``): the contracts of
    ``HipEncoderTrainer``, the kernels of the MAE engine's ``_block_fwd16`` / ``_block_bwd16`` (non-grouped form).  Every Linear runs
    on the LDS-DMA GEMM with bf16 operands written by their producers — LayerNorm's bf16 output, the qkv GEMM's bf16 q | k | v, the
    attention's ``o_16``, fc1's bf16 GELU and bf16 GELU' — and its backward is one paired launch (input gradient + weight gradient)
    whose dy operand the previous launch wrote in bf16.  Bias gradients ride on those launches (``dy_colsum`` / ``dx_colsum``).

    Kept per token row and block: x_in and xmid in fp32 (LayerNorm backward), o in fp32 (attention backward) and, in bf16, y1, q | k | v,
    o, y2, GELU' and the activation: 40 D bytes against 64 D, plus the row statistics.

    The weight-gradient half of a paired launch reduces over ``Mpad`` rows (M rounded up to 64) and needs rows M .. Mpad - 1 of both
    operands to be zero.  No such buffer outlives a call: each is allocated with ``Mpad`` rows in the call that fills it (``_z16``) and
    the pad rows of all of them are zeroed there by ONE multi-tensor launch in front of the call's first kernel (``_zero_pads``), so a
    smaller batch after a larger one finds nothing stale.  Frozen Linear: ``dw = NULL``, the
    launch computes the input gradient alone; its bias gradient then comes from a launch that does not depend on the weight
    gradient (fc1: the column sums of fc2's input-gradient epilogue; qkv: the attention backward's)."""

    def __init__(self, module, precision: str = 'bf16'):
        super().__init__(module, precision)
        why = act16_refusal_for(module, precision)
        if why:
            raise VitaeError(why)
        self.act16 = True
        self.stats['route'] = 'bf16-activations'
        self._pads = []

    def _workspace(self, B: int, L: int):
        if self._B != self.device:
            self._B = self.device
            # split-K scratch of the LDS-DMA family: its ticket words start as zero and every launch leaves them zero (HipEncoder._alloc)
            self.buf = {'ws16': torch.zeros(self.WS_FLOATS, dtype=torch.float32, device=self.device)}
        if ('ids', B) not in self.buf:
            self.buf['ids', B] = torch.arange(L, dtype=torch.int32, device=self.device).repeat(B, 1).contiguous()
        return self.buf['ids', B]

    def _e16(self, *shape):
        return torch.empty(*shape, dtype=torch.bfloat16, device=self.device)

    def _z16(self, M, Mpad, W):
        """A bf16 GEMM operand of M rows in a buffer of Mpad: the producers write rows < M only; the pad rows wait for ``_zero_pads``."""
        t = self._e16(Mpad, W)
        if Mpad > M:
            self._pads.append(t[M:])
        return t

    def _zero_pads(self):
        """Zero the pad rows of every operand allocated since the last call, in one launch (a memset each was ~50 launches per ViT-B
        forward)."""
        if self._pads:
            torch._foreach_zero_(self._pads)
            self._pads = []

    # ------------------------------------------------------------------ forward
    def _ln16(self, x, pre, y16, mean, rstd, M, D):
        lib.vitae_layernorm_fwd(_ptr(x), _ptr(self._param(pre + 'weight')), _ptr(self._param(pre + 'bias')), None, _ptr(y16),
                                _ptr(mean), _ptr(rstd), M, D, self.eps, self.stream)

    def _block_bufs(self, B, N, D, H):
        """What one block keeps, except its input."""
        f, z, M, heads = self._f, self._z16, B * N, self.m.num_heads
        Mp = (M + 63) // 64 * 64
        return {'mean1': f(M), 'rstd1': f(M), 'y1_16': z(M, Mp, D), 'qkv_16': self._e16(M, 3 * D), 'o': f(M, D),
                'o_16': z(M, Mp, D), 'lse': f(B * heads * N), 'xmid': f(M, D), 'mean2': f(M), 'rstd2': f(M), 'y2_16': z(M, Mp, D),
                'dgelu_16': self._e16(M, H), 'act_16': z(M, Mp, H)}

    def _block_run(self, q, k, x_in, B, N, D, H):
        """One block into the buffers ``k`` -> its output."""
        M, heads = B * N, self.m.num_heads
        k['x_in'] = x_in
        x_out = self._f(M, D)
        self._ln16(x_in, q + 'norm1.', k['y1_16'], k['mean1'], k['rstd1'], M, D)
        self._g16(k['y1_16'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', M, 3 * D, D, y16=k['qkv_16'])
        lib.vitae_sdpa_mfma_fwd_bf16in(_ptr(k['qkv_16']), _ptr(k['o']), _ptr(k['o_16']), _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        self._g16(k['o_16'], q + 'attn.proj.weight', q + 'attn.proj.bias', M, D, D, y=k['xmid'], res=x_in)
        self._ln16(k['xmid'], q + 'norm2.', k['y2_16'], k['mean2'], k['rstd2'], M, D)
        # aux <- bf16 GELU'(pre-activation): what the fc2 input-gradient epilogue multiplies by
        self._g16(k['y2_16'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', M, H, D, y16=k['act_16'],
                  epi=EPI_GELU | EPI_AUX_BF16 | EPI_AUX_DERIV, aux=k['dgelu_16'])
        self._g16(k['act_16'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', M, D, H, y=x_out, res=k['xmid'])
        return x_out

    def forward_keep(self, x: torch.Tensor, needs: Dict[str, bool]):
        """-> (features [B, D], kept): ``kept`` is what ``backward`` needs, owned by the caller."""
        m = self.m
        B, C, Lz, Hy, Wx, ps = self._begin(x)
        L, D, H, P = m.patch_embed.num_patches, m.embed_dim, self.hidden, self.P
        N, M, depth = L + 1, B * (L + 1), len(m.blocks)
        why = act16_refusal_for(m, self.precision, in_chans=C)
        if why:         # (the input's channel count is only known here)
            raise VitaeError(why)
        ids = self._workspace(B, L)
        f, st = self._f, self.stream
        embed, lo = self.lowest_trainable(needs, depth)
        xc = x.detach().contiguous().float()
        T = B * L
        patches16, tok, cur = self._z16(T, (T + 63) // 64 * 64, P), f(T, D), f(M, D)
        # every buffer of the call before its first launch: the blocks the backward will walk keep their own, the ones below share one set
        blocks = {i: self._block_bufs(B, N, D, H) for i in range(min(lo, depth), depth)}
        shared = self._block_bufs(B, N, D, H) if min(lo, depth) > 0 else None
        self._zero_pads()
        lib.vitae_gather_patches(_ptr(xc), _ptr(ids), None, _ptr(patches16), B, C, Lz, Hy, Wx, ps, L, st)
        self._g16(patches16, 'patch_embed.proj.weight', 'patch_embed.proj.bias', T, D, P, y=tok)
        lib.vitae_encoder_assemble_fwd(_ptr(tok), _ptr(self._param('cls_token')), _ptr(self._param('pos_embed')), _ptr(ids),
                                       _ptr(cur), B, L, L, D, st)
        for i in range(depth):
            cur = self._block_run(f'blocks.{i}.', blocks.get(i, shared), cur, B, N, D, H)
        pool, feat, mean, rstd = f(B, D), f(B, D), f(B), f(B)
        if m.global_pool:
            lib.vitae_mean_pool_tokens(_ptr(cur), _ptr(pool), B, N, D, 1, st)
            self._ln_keep(pool, 'fc_norm.', feat, mean, rstd, B, D)
        else:
            pool.copy_(cur.view(B, N, D)[:, 0])
            self._ln_keep(pool, 'norm.', feat, mean, rstd, B, D)
        kept = {'geom': (B, L, D, H, P), 'needs': dict(needs), 'params': self.sd, 'embed': embed, 'lo': lo, 'blocks': blocks,
                'versions': {n: p._version for n, p in self.sd.items() if not n.startswith('head.')},
                'patches_16': patches16 if needs.get('patch_embed.proj.weight') else None, 'pool': pool, 'mean': mean, 'rstd': rstd}
        self.stats['forwards'] += 1
        self.stats['kept_bytes'] = (sum(t.numel() * t.element_size() for kb in blocks.values() for t in kb.values())
                                    + sum(t.numel() * t.element_size() for t in (kept['patches_16'], pool, mean, rstd) if t is not None))
        return feat, kept

    # ------------------------------------------------------------------ backward
    def _pair(self, grads, needs, dy16, wname, x16, M, Mpad, N, K, dx=None, dx16=None, epi=EPI_NONE, aux=None, dx_colsum=None,
              dy_colsum=None):
        """Backward of y = x W^T + b on bf16 operands, dy16 [Mpad, N]: dx / dx16 [M, K] = epi(dy16 W16) and, for a trainable weight,
        dW = dy16^T x16 in the same launch.  ``dx_colsum`` / ``dy_colsum`` (zeroed by the caller) collect column sums of dx / dy16."""
        ws = self.buf['ws16']
        key = ('p', M, N, K)
        s = self._split.get(key)
        if s is None:
            s = lib.vitae_linear_bwd_pair_pick_split_k(M, Mpad, N, K)
            while s > 1 and lib.vitae_gemm_glds_ws_floats(M, K, s) > ws.numel():
                s -= 1
            self._split[key] = s
        dw = None
        if needs.get(wname):
            dw = grads[wname] = torch.empty_like(self._param(wname))
        assert dw is not None or dy_colsum is None      # the input-gradient-only form takes no column sums of dy16
        lib.vitae_linear_bwd_pair_glds(_ptr(dy16), self._bf16(wname), _ptr(x16), _ptr(dx), _ptr(dx16), _ptr(dw), None, M, Mpad, N, K,
                                       epi, _ptr(aux), _ptr(dx_colsum), _ptr(dy_colsum), 0, 0, s, ws.data_ptr(), ws.numel(), self.stream)

    def _ln_bwd16(self, grads, needs, dy, x, pre, mean, rstd, dx, dx16, dx_colsum, M, D):
        dw, db = self._z(D), self._z(D)             # the launcher adds its column partials
        lib.vitae_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(self._param(pre + 'weight')), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dw),
                                _ptr(db), _ptr(dx16), _ptr(dx_colsum), M, D, 1, self.stream)
        if needs.get(pre + 'weight'):
            grads[pre + 'weight'] = dw
        if needs.get(pre + 'bias'):
            grads[pre + 'bias'] = db

    def backward(self, kept, dfeat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """d loss / d features [B, D] -> {parameter name: gradient} for the trainable parameters of the encoder."""
        m = self.m
        B, L, D, H, P = kept['geom']
        N, M, depth, heads = L + 1, B * (L + 1), len(m.blocks), m.num_heads
        Mp = (M + 63) // 64 * 64
        self.device = dfeat.device
        self.stream = torch.cuda.current_stream(dfeat.device).cuda_stream
        self.sd = kept['params']
        stale = [n for n, v in kept['versions'].items() if self.sd[n]._version != v]
        if stale:       # the backward reads the bf16 weight copies again (keyed by version): they must be the ones the forward used
            raise VitaeError(f'parameters were modified in place between forward and backward: {stale[:3]} ...')
        self._workspace(B, L)
        needs, f, st = kept['needs'], self._f, self.stream
        grads: Dict[str, torch.Tensor] = {}
        dfeat = dfeat.contiguous().float()
        dpool = f(B, D)
        self._ln_bwd(grads, needs, dfeat, kept['pool'], 'fc_norm.' if m.global_pool else 'norm.', kept['mean'], kept['rstd'],
                     dpool, B, D, 0)
        self.stats['backwards'] += 1
        embed, lo = kept['embed'], kept['lo']
        if not embed and lo >= depth:
            return grads

        def bias(name):     # a bias gradient that launches ADD column sums to; None for a frozen bias
            if needs.get(name):
                grads[name] = self._z(self._param(name).numel())
                return grads[name]
            return None

        # the hand-over from the head: dx, its bf16 copy with zero pad rows, and the top block's fc2 bias gradient (overwritten)
        dx, dx16 = f(M, D), self._e16(Mp, D)
        fc2_b = bias(f'blocks.{depth - 1}.mlp.fc2.bias') if depth else None
        lib.vitae_token_select_bwd16(_ptr(dpool), _ptr(dx), _ptr(dx16), _ptr(fc2_b), B, N, Mp, D, 1 if m.global_pool else 0, st)
        T = B * L
        Tp = (T + 63) // 64 * 64
        if depth > lo:
            dh16, dqkv16 = self._z16(M, Mp, H), self._z16(M, Mp, 3 * D)
            dy, do, delta = f(M, D), f(M, D), f(B * heads * N)
        dtok16 = self._z16(T, Tp, D) if (embed and needs.get('patch_embed.proj.weight')) else None
        self._zero_pads()
        for i in range(depth - 1, lo - 1, -1):
            q, k = f'blocks.{i}.', kept['blocks'][i]
            # fc1's bias gradient colsum(dh): beside fc1's weight gradient when there is one, else from fc2's input-gradient epilogue
            fc1_b = bias(q + 'mlp.fc1.bias')
            by_w = bool(needs.get(q + 'mlp.fc1.weight'))
            self._pair(grads, needs, dx16, q + 'mlp.fc2.weight', k['act_16'], M, Mp, D, H, dx16=dh16,
                       epi=EPI_DGELU | EPI_AUX_BF16 | EPI_AUX_DERIV, aux=k['dgelu_16'], dx_colsum=None if by_w else fc1_b)
            self._pair(grads, needs, dh16, q + 'mlp.fc1.weight', k['y2_16'], M, Mp, H, D, dx=dy, dy_colsum=fc1_b if by_w else None)
            self._ln_bwd16(grads, needs, dy, k['xmid'], q + 'norm2.', k['mean2'], k['rstd2'], dx, dx16, bias(q + 'attn.proj.bias'), M, D)
            self._pair(grads, needs, dx16, q + 'attn.proj.weight', k['o_16'], M, Mp, D, D, dx=do)
            # qkv's bias gradient colsum(dqkv): beside its weight gradient, or collected by the attention backward for a frozen weight
            qkv_b = bias(q + 'attn.qkv.bias')
            by_w = bool(needs.get(q + 'attn.qkv.weight'))
            lib.vitae_sdpa_mfma_bwd_bf16in(_ptr(k['qkv_16']), _ptr(k['o']), _ptr(do), _ptr(k['lse']), None, _ptr(dqkv16),
                                           None if by_w else _ptr(qkv_b), _ptr(delta), B, N, heads, self.hd, st)
            self._pair(grads, needs, dqkv16, q + 'attn.qkv.weight', k['y1_16'], M, Mp, 3 * D, D, dx=dy, dy_colsum=qkv_b if by_w else None)
            # norm1 leaves the output gradient of block i - 1: fp32, bf16, and its column sums = that block's fc2 bias gradient
            below = i > lo
            self._ln_bwd16(grads, needs, dy, k['x_in'], q + 'norm1.', k['mean1'], k['rstd1'], dx, dx16 if below else None,
                           bias(f'blocks.{i - 1}.mlp.fc2.bias') if below else None, M, D)
        if embed:
            want_w, want_b = needs.get('patch_embed.proj.weight'), needs.get('patch_embed.proj.bias')
            pos = self._param('pos_embed')
            dpos = torch.empty_like(pos) if (needs.get('pos_embed') or want_b) else None
            dcls = grads['cls_token'] = torch.empty_like(self._param('cls_token')) if needs.get('cls_token') else None
            if needs.get('pos_embed'):
                grads['pos_embed'] = dpos
            lib.vitae_vit_assemble_bwd(_ptr(dx), None, _ptr(dtok16), _ptr(dpos), _ptr(dcls), B, L, D, 0, st)
            if want_b:
                # colsum(dtok) = sum over the patch rows of dpos (dpos[n] = sum_b dx[b, n]): L rows instead of B L
                db = grads['patch_embed.proj.bias'] = self._z(D)
                lib.vitae_colsum_accum(dpos.data_ptr() + 4 * D, D, _ptr(db), L, D, st)
            if want_w:
                # dW[D, P] = dtok16^T @ patches16 (both row-contiguous bf16, reduced over the padded token count)
                dw = grads['patch_embed.proj.weight'] = torch.empty_like(self._param('patch_embed.proj.weight'))
                lib.vitae_gemm_glds(0, 0, _ptr(dtok16), D, _ptr(kept['patches_16']), P, _ptr(dw), P, None, P, D, P, Tp, None, None, 0,
                                    EPI_NONE, None, 0, 0, 1, None, None, st)
        return {n: g for n, g in grads.items() if g is not None}

"""The all-token encoder of ``VisionTransformer3D`` on MI355X (reference model/vit.py:265-284): feature extraction (driven by
utils/feature_extraction.py:9-45 after pre-training) and fine-tuning (post_training_utils/fine_tune_epoch.py:34-100).

Same kernels as the training engine's encoder, unmasked (every patch is kept, N = L + 1 tokens):
patch gather -> patch-embedding GEMM -> cls/pos assembly -> depth x [LN, qkv, attention, proj(+res), LN,
fc1+GELU, fc2(+res)] -> global-pool mean + fc_norm, or norm of the cls rows.

Two activation routes, each with ONE block forward (``HipEncoder._block32`` / ``_block16``) over a dictionary of buffers:
  fp32 activations  every Linear on the generic launcher (exact-fp32 MFMA, split bf16 hi + lo, or bf16 MFMA on fp32 activations);
  bf16 activations  GEMM operands in bf16 written by their producers, every Linear on the LDS-DMA GEMM.  ``act16_refusal`` is the
                    rule: bf16 precision (the counterpart of the reference's ``torch.cuda.amp.autocast()``), all contraction lengths
                    multiples of 64, an MFMA head size.

``HipEncoder`` is inference: it takes the bf16 route whenever the rule allows, keeps nothing for a backward and runs every block on
one cached set of buffers, two activation buffers ping-ponging.  ``HipEncoderTrainer`` (fp32 route) and ``HipEncoderTrainer16`` (bf16
route) share the frame ``_Trainer``: the same embedding, block forward and pooling on per-call buffers that the caller keeps, and a
``backward`` each, which is the place to read a route's launch order.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import torch

from ._abi import CONSTS as _C, VitaeError, lib
from ._launch import EPI_AUX_BF16, EPI_AUX_DERIV, EPI_DGELU, EPI_GELU, EPI_NONE, PREC, fit_split, pad64 as _pad64, ptr as _ptr
from .shadow import store_of

_EMBED = ('cls_token', 'pos_embed', 'patch_embed.proj.weight', 'patch_embed.proj.bias')


def act16_refusal(precision, embed_dim, hidden, patch_dim, head_dim):
    """Why the bf16-activation route does not serve this model (None: it does): bf16 arithmetic, every contraction length a multiple
    of the LDS-DMA GEMM's 64-wide k-tile, an MFMA head size."""
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


class HipEncoder:
    """Sequences the encoder kernels for one ``VisionTransformer3D`` instance (weights are read from the module's parameters at call
    time; bf16 copies live in the model's shadow store, shadow.py) and runs them for inference.  The launch helpers of both routes live here;
    ``self.buf`` holds the split-K scratch of the route in use (``'ws'``: generic launchers, ``'ws16'``: LDS-DMA family, whose ticket
    words start as zero and are left zero by every launch) and, for inference, the cached activation buffers."""

    def __init__(self, module, precision: str = 'fp32'):
        if precision not in PREC:
            raise VitaeError(f'unknown precision {precision!r}')
        lib.load()
        self.m = module
        self.precision, self.prec = precision, PREC[precision]
        self._B = None          # (batch size, device) the inference buffers were made for
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
        """Address of the bf16 copy of parameter ``name``: its slot in the model's shadow store (shadow.py), cast here when the slot does
        not hold the parameter as it is now.  The multi-tensor updaters keep a current slot current, so a steady step casts nothing."""
        p = self._param(name)
        slot = store_of(self.m).slot(p)
        if not slot.current():
            lib.vitae_cast_bf16(p.data_ptr(), slot.address(), p.numel(), self.stream)
            slot.mark()
        return slot.address()

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int):
        """The buffers of an inference forward at batch size B, cached until B or the device changes.  One set serves every block,
        so the two LayerNorms of a block share their output and statistics (``y1`` is ``y2``, ``mean1`` is ``mean2``)."""
        m = self.m
        L, D, H, P = m.patch_embed.num_patches, m.embed_dim, self.hidden, self.P
        M = B * (L + 1)
        if self._B == (B, self.device):
            return
        self._B = (B, self.device)
        dev = self.device
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        b = self.buf = {}
        b['ids'] = torch.arange(L, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
        b['tok'] = f(B * L, D)
        b['xa'], b['xb'], b['xmid'] = f(M, D), f(M, D), f(M, D)
        b['qkv'], b['o'], b['lse'] = f(M, 3 * D), f(M, D), f(B * m.num_heads * (L + 1))
        b['mean1'], b['rstd1'] = f(M), f(M)
        b['hpre'] = f(M, H)
        b['pool'], b['feat'] = f(B, D), f(B, D)
        if self.act16:
            z16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
            b['patches_16'] = z16(B * L, P)
            b['y1_16'], b['o_16'], b['act_16'] = z16(M, D), z16(M, D), z16(M, H)
            b['y2_16'] = b['y1_16']
            b['ws16'] = torch.zeros(1 << 22, dtype=torch.float32, device=dev)
        else:
            b['patches'], b['y1'], b['act'] = f(B * L, P), f(M, D), f(M, H)
            b['y2'] = b['y1']
            b['ws'] = f(1 << 22)
        b['mean2'], b['rstd2'] = b['mean1'], b['rstd1']

    # ------------------------------------------------------------------ launch helpers
    def _g16(self, x16, wname, bname, M, N, K, y=None, y16=None, epi=EPI_NONE, aux=None, res=None):
        """y / y16 [M, N] = epi(x16 W16^T + b) (+ res) on the LDS-DMA GEMM; a GELU epilogue cannot be split."""
        ws, key = self.buf['ws16'], ('g', M, N, K, epi)
        s = self._split.get(key) or fit_split(
            self._split, key, lambda: 1 if (epi & 15) == EPI_GELU else lib.vitae_gemm_glds_pick_split_k(M, N, K),
            lambda s: lib.vitae_gemm_glds_ws_floats(M, N, s), ws.numel())
        lib.vitae_gemm_glds(1, 1, _ptr(x16), K, self._bf16(wname), K, _ptr(y), N, _ptr(y16), N, M, N, K,
                            _ptr(self._param(bname)), _ptr(res), N, epi, _ptr(aux), N, 0, s, ws.data_ptr(), None, self.stream)

    def _lin(self, x, wname, bname, y, M, N, K, epi=EPI_NONE, aux=None, res=None):
        """y [M, N] = epi(x W^T + b) (+ res) on the generic launcher; any epilogue forces one split."""
        ws, key = self.buf['ws'], ('l', M, N, K, epi)
        s = self._split.get(key) or fit_split(
            self._split, key, lambda: 1 if epi != EPI_NONE else lib.vitae_gemm_pick_split_k(M, N, K), lambda s: s * M * N, ws.numel())
        lib.vitae_linear_fwd(self.prec, _ptr(x), _ptr(self._param(wname)), _ptr(self._param(bname)), _ptr(y), M, N, K, epi,
                             _ptr(aux), _ptr(res), s, ws.data_ptr(), self.stream)

    def _ln(self, x, pre, y, y16, mean, rstd, M, D):
        lib.vitae_layernorm_fwd(_ptr(x), _ptr(self._param(pre + 'weight')), _ptr(self._param(pre + 'bias')), _ptr(y), _ptr(y16),
                                _ptr(mean), _ptr(rstd), M, D, self.eps, self.stream)

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

    def _embed(self, xc, vol, ids, patches, patches16, tok, x0):
        """Volume ``xc`` of geometry ``vol`` (what ``_begin`` returned) -> token rows ``x0`` [B (L + 1), D].  The patch operand is
        ``patches`` (fp32, generic launcher) or ``patches16`` (bf16, LDS-DMA GEMM); the other one is None."""
        B, L, D = vol[0], self.m.patch_embed.num_patches, self.m.embed_dim
        lib.vitae_gather_patches(_ptr(xc), _ptr(ids), _ptr(patches), _ptr(patches16), *vol, L, self.stream)
        if patches16 is not None:
            self._g16(patches16, 'patch_embed.proj.weight', 'patch_embed.proj.bias', B * L, D, self.P, y=tok)
        else:
            self._lin(patches, 'patch_embed.proj.weight', 'patch_embed.proj.bias', tok, B * L, D, self.P)
        lib.vitae_encoder_assemble_fwd(_ptr(tok), _ptr(self._param('cls_token')), _ptr(self._param('pos_embed')), _ptr(ids),
                                       _ptr(x0), B, L, L, D, self.stream)

    def _block32(self, q, k, x_in, x_out, aux_epi, B, N, D, H):
        """Block ``q`` on fp32 activations: x_in -> x_out through the buffers ``k``.  ``aux_epi``: what fc1 leaves in ``hpre`` beside
        its GELU (nothing more: the pre-activation; ``EPI_AUX_DERIV``: GELU' of it, what a backward multiplies by)."""
        M, heads = B * N, self.m.num_heads
        self._ln(x_in, q + 'norm1.', k['y1'], None, k['mean1'], k['rstd1'], M, D)
        self._lin(k['y1'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', k['qkv'], M, 3 * D, D)
        if self.prec == PREC['bf16'] and self.hd in (32, 64):
            lib.vitae_sdpa_mfma_fwd(_ptr(k['qkv']), _ptr(k['o']), None, _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        else:
            lib.vitae_sdpa_fwd(_ptr(k['qkv']), _ptr(k['o']), _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        self._lin(k['o'], q + 'attn.proj.weight', q + 'attn.proj.bias', k['xmid'], M, D, D, res=x_in)
        self._ln(k['xmid'], q + 'norm2.', k['y2'], None, k['mean2'], k['rstd2'], M, D)
        self._lin(k['y2'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', k['act'], M, H, D, epi=EPI_GELU | aux_epi, aux=k['hpre'])
        self._lin(k['act'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', x_out, M, D, H, res=k['xmid'])

    def _block16(self, q, k, x_in, x_out, qkv16, aux_epi, aux_key, B, N, D, H):
        """Block ``q`` on bf16 activations: x_in -> x_out through the buffers ``k``.  ``qkv16``: q | k | v are kept in bf16
        (``qkv_16``) and the attention reads them there; otherwise it reads the fp32 ``qkv``.  fc1 leaves in ``k[aux_key]`` what
        ``aux_epi`` says beside its GELU (nothing more: the fp32 pre-activation; ``EPI_AUX_BF16 | EPI_AUX_DERIV``: bf16 GELU' of it,
        what the fc2 input-gradient epilogue multiplies by)."""
        M, heads = B * N, self.m.num_heads
        self._ln(x_in, q + 'norm1.', None, k['y1_16'], k['mean1'], k['rstd1'], M, D)
        if qkv16:
            self._g16(k['y1_16'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', M, 3 * D, D, y16=k['qkv_16'])
            lib.vitae_sdpa_mfma_fwd_bf16in(_ptr(k['qkv_16']), _ptr(k['o']), _ptr(k['o_16']), _ptr(k['lse']), B, N, heads, self.hd,
                                           self.stream)
        else:
            self._g16(k['y1_16'], q + 'attn.qkv.weight', q + 'attn.qkv.bias', M, 3 * D, D, y=k['qkv'])
            lib.vitae_sdpa_mfma_fwd(_ptr(k['qkv']), _ptr(k['o']), _ptr(k['o_16']), _ptr(k['lse']), B, N, heads, self.hd, self.stream)
        self._g16(k['o_16'], q + 'attn.proj.weight', q + 'attn.proj.bias', M, D, D, y=k['xmid'], res=x_in)
        self._ln(k['xmid'], q + 'norm2.', None, k['y2_16'], k['mean2'], k['rstd2'], M, D)
        self._g16(k['y2_16'], q + 'mlp.fc1.weight', q + 'mlp.fc1.bias', M, H, D, y16=k['act_16'], epi=EPI_GELU | aux_epi, aux=k[aux_key])
        self._g16(k['act_16'], q + 'mlp.fc2.weight', q + 'mlp.fc2.bias', M, D, H, y=x_out, res=k['xmid'])

    def _pool_norm(self, x, pool, feat, mean, rstd, B, N, D):
        """Token rows x -> features [B, D]; the final norm's statistics go to ``mean`` / ``rstd``."""
        if self.m.global_pool:
            lib.vitae_mean_pool_tokens(_ptr(x), _ptr(pool), B, N, D, 1, self.stream)
            self._ln(pool, 'fc_norm.', feat, None, mean, rstd, B, D)
        else:
            # LayerNorm is row-wise: normalising only the cls rows equals norm(x)[:, 0] (model/vit.py:281-282)
            pool.copy_(x.view(B, N, D)[:, 0])
            self._ln(pool, 'norm.', feat, None, mean, rstd, B, D)

    @torch.no_grad()
    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        m = self.m
        vol = self._begin(x)
        B, N, D, H = vol[0], m.patch_embed.num_patches + 1, m.embed_dim, self.hidden
        self.act16 = act16_refusal(self.precision, D, H, self.P, self.hd) is None
        self._alloc(B)
        b = self.buf
        self._embed(x.contiguous().float(), vol, b['ids'], b.get('patches'), b.get('patches_16'), b['tok'], b['xa'])
        cur, nxt = b['xa'], b['xb']
        for i in range(len(m.blocks)):
            if self.act16:
                self._block16(f'blocks.{i}.', b, cur, nxt, False, EPI_NONE, 'hpre', B, N, D, H)
            else:
                self._block32(f'blocks.{i}.', b, cur, nxt, EPI_NONE, B, N, D, H)
            cur, nxt = nxt, cur
        self._pool_norm(cur, b['pool'], b['feat'], b['mean1'], b['rstd1'], B, N, D)
        return b['feat'].clone()


class _Trainer(HipEncoder):
    """What the two fine-tuning routes share.  ``forward_keep`` runs the inference launch sequence on buffers allocated per call and
    returns, beside the features, what ``backward`` reads: the caller owns it (and hangs it on the autograd context), so any number of
    forwards may precede a backward.  Only split-K scratch and the patch index table live on the trainer.  Gradients are produced for
    the parameters named in ``needs`` only: a frozen Linear has no weight-gradient launch, and blocks below the lowest trainable
    parameter are neither kept (they run on one shared set of buffers) nor walked.  ``backward`` is the route's own, after
    ``_backward_head``.  ``stats`` counts the calls and the bytes the last forward kept (tests and tools/finetune_bench.py read it).

    A route supplies ``ROUTE``, ``act16``, ``SCRATCH`` / ``SCRATCH_ZEROED`` (its split-K scratch in ``buf`` and whether that starts as
    zero), ``_refusal``, ``_patch_operand``, ``_block_bufs``, ``_block`` and ``backward``; the bf16 route also ``_zero_pads``."""

    WS_FLOATS = 1 << 24        # split-K scratch, 64 MiB (as the training engine's)

    def __init__(self, module, precision):
        super().__init__(module, precision)
        self.stats = {'forwards': 0, 'backwards': 0, 'kept_bytes': 0, 'route': self.ROUTE}

    def _workspace(self, B: int, L: int):
        """Scratch (it does not depend on the batch: forwards of different sizes may interleave) -> the patch index table of batch B."""
        ws = self.buf.get(self.SCRATCH)
        if ws is None or ws.device != self.device:
            make = torch.zeros if self.SCRATCH_ZEROED else torch.empty
            self.buf = {self.SCRATCH: make(self.WS_FLOATS, dtype=torch.float32, device=self.device)}
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

    def forward_keep(self, x: torch.Tensor, needs: Dict[str, bool]):
        """-> (features [B, D], kept): ``kept`` is what ``backward`` needs, owned by the caller."""
        m = self.m
        vol = self._begin(x)
        B, C = vol[0], vol[1]
        L, D, H, P = m.patch_embed.num_patches, m.embed_dim, self.hidden, self.P
        N, M, depth = L + 1, B * (L + 1), len(m.blocks)
        why = self._refusal(C)
        if why:         # (the input's channel count is only known here)
            raise VitaeError(why)
        ids = self._workspace(B, L)
        f = self._f
        embed, lo = self.lowest_trainable(needs, depth)
        xc = x.detach().contiguous().float()
        patches, patches16 = self._patch_operand(B * L, P)
        tok, cur = f(B * L, D), f(M, D)
        # the blocks the backward will walk keep their own buffers, the ones below share one set
        blocks, shared = {}, None
        if self.act16:          # every Mpad-row operand of the call before its first launch, for one zeroing of all pad rows
            blocks = {i: self._block_bufs(B, N, D, H) for i in range(min(lo, depth), depth)}
            shared = self._block_bufs(B, N, D, H) if min(lo, depth) > 0 else None
            self._zero_pads()
        self._embed(xc, vol, ids, patches, patches16, tok, cur)
        for i in range(depth):
            x_in, cur = cur, f(M, D)
            k = blocks.get(i) if i >= lo else shared
            if k is None:       # fp32 route: allocated block by block, while the GPU runs the launches already issued
                k = self._block_bufs(B, N, D, H)
                if i >= lo:
                    blocks[i] = k
                else:
                    shared = k
            k['x_in'] = x_in
            self._block(f'blocks.{i}.', k, x_in, cur, B, N, D, H)
        pool, feat, mean, rstd = f(B, D), f(B, D), f(B), f(B)
        self._pool_norm(cur, pool, feat, mean, rstd, B, N, D)
        kept = {'geom': (B, L, D, H, P), 'needs': dict(needs), 'params': self.sd, 'embed': embed, 'lo': lo, 'blocks': blocks,
                'versions': {n: p._version for n, p in self.sd.items() if not n.startswith('head.')},
                'patches': (patches if patches16 is None else patches16) if needs.get('patch_embed.proj.weight') else None,
                'pool': pool, 'mean': mean, 'rstd': rstd}
        self.stats['forwards'] += 1
        self.stats['kept_bytes'] = (sum(t.numel() * t.element_size() for kb in blocks.values() for t in kb.values())
                                    + sum(t.numel() * t.element_size() for t in (kept['patches'], pool, mean, rstd) if t is not None))
        return feat, kept

    def _colsum(self, dy_ptr, ld, out, M, N):
        """out[n] += sum_m dy[m, n] (a bias gradient); in a fixed order when the module asks for it (``ordered_norm_grads``, see _ln_bwd)."""
        if getattr(self.m, 'ordered_norm_grads', False):
            ws = self._f(int(lib.vitae_colsum_ordered_ws_floats(M, N)))
            lib.vitae_colsum_ordered(dy_ptr, ld, _ptr(out), _ptr(ws), M, N, self.stream)
        else:
            lib.vitae_colsum_accum(dy_ptr, ld, _ptr(out), M, N, self.stream)

    def _ln_bwd(self, grads, needs, dy, x, pre, mean, rstd, dx, M, D, dx_accumulate, dx16=None, dx_colsum=None):
        """LayerNorm backward: dx (+)= ..., optionally its bf16 copy ``dx16`` and its column sums added to ``dx_colsum``."""
        dw, db = self._z(D), self._z(D)             # the launcher adds its column partials
        if getattr(self.m, 'ordered_norm_grads', False):
            if D % 4 or (D > 768 and D != 1024):        # (no quiet return to the atomic form: the flag promises reproducible sums)
                raise VitaeError(f'ordered_norm_grads: the atomic-free LayerNorm backward serves D % 4 == 0 up to 768, and 1024 (got {D})')
            # no atomics (set by other_baselines.mocov3.moco.builder.MoCo on its base encoder): every workgroup leaves its partials
            # as a record and one reduce launch adds the records in a fixed order, so these gradients reproduce bit for bit
            vec = D in (256, 512, 768, 1024)
            G = lib.vitae_layernorm_bwd_part_records(M) if vec else -(-M // _C['VITAE_LN_PART_ANY_ROWS'])
            part = self._f(G * 3 * D)
            (lib.vitae_layernorm_bwd_part if vec else lib.vitae_layernorm_bwd_part_any)(
                _ptr(dy), _ptr(x), _ptr(self._param(pre + 'weight')), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(part), _ptr(dx16), M, D,
                dx_accumulate, self.stream)
            one = lambda v, t=ctypes.c_void_p: (t * 1)(v)
            lib.vitae_ln_grad_reduce(1, one(part.data_ptr()), one(dw.data_ptr()), one(db.data_ptr()), one(_ptr(dx_colsum)),
                                     one(G, ctypes.c_int), one(D, ctypes.c_int), self.stream)
        else:
            lib.vitae_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(self._param(pre + 'weight')), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dw),
                                    _ptr(db), _ptr(dx16), _ptr(dx_colsum), M, D, dx_accumulate, self.stream)
        if needs.get(pre + 'weight'):
            grads[pre + 'weight'] = dw
        if needs.get(pre + 'bias'):
            grads[pre + 'bias'] = db

    def _backward_head(self, kept, dfeat: torch.Tensor):
        """How every ``backward`` begins: geometry of the call, the stale-parameter check, the final norm's backward.
        -> (grads so far, dpool [B, D]; None when no block and no embedding parameter is trainable: the backward is complete)."""
        B, L, D, H, P = kept['geom']
        self.device = dfeat.device
        self.stream = torch.cuda.current_stream(dfeat.device).cuda_stream
        self.sd = kept['params']
        stale = [n for n, v in kept['versions'].items() if self.sd[n]._version != v]
        # the backward reads the weights (and their bf16 copies, keyed by version) again: they must be the ones the forward used (as
        # autograd checks for its own ops)
        if stale:
            raise VitaeError(f'parameters were modified in place between forward and backward: {stale[:3]} ...')
        self._workspace(B, L)
        grads: Dict[str, torch.Tensor] = {}
        dfeat = dfeat.contiguous().float()
        dpool = self._f(B, D)
        self._ln_bwd(grads, kept['needs'], dfeat, kept['pool'], 'fc_norm.' if self.m.global_pool else 'norm.', kept['mean'],
                     kept['rstd'], dpool, B, D, 0)
        self.stats['backwards'] += 1
        if not kept['embed'] and kept['lo'] >= len(self.m.blocks):
            return grads, None
        return grads, dpool


class HipEncoderTrainer(_Trainer):
    """Fine-tuning on fp32 activations and the generic Linear launchers (any precision): ``backward`` walks the blocks from the top
    in the launch order of ``HipMAEEngine._block_bwd`` — separate input-gradient, weight-gradient and column-sum launches, eager on
    the current stream, no side streams, no graph capture.  ``HipEncoderTrainer16`` is the bf16-activation route."""

    ROUTE, SCRATCH, SCRATCH_ZEROED = 'fp32-activations', 'ws', False
    act16 = False

    def __init__(self, module, precision: str = 'fp32'):
        super().__init__(module, precision)

    def _refusal(self, in_chans):
        return 'embed_dim must be a multiple of 4' if self.m.embed_dim % 4 else None

    def _patch_operand(self, T, P):
        return self._f(T, P), None

    def _block_bufs(self, B, N, D, H):
        """What one block keeps, except its input."""
        f, M = self._f, B * N
        return {'mean1': f(M), 'rstd1': f(M), 'y1': f(M, D), 'qkv': f(M, 3 * D), 'o': f(M, D), 'lse': f(B * self.m.num_heads * N),
                'xmid': f(M, D), 'mean2': f(M), 'rstd2': f(M), 'y2': f(M, D), 'hpre': f(M, H), 'act': f(M, H)}

    def _block(self, q, k, x_in, x_out, B, N, D, H):
        self._block32(q, k, x_in, x_out, EPI_AUX_DERIV, B, N, D, H)

    # ------------------------------------------------------------------ backward
    def _split_bwd(self, M, N, K):
        """Split of the reduction (length K) of a backward GEMM with an [M, N] result, fitted to the scratch buffer."""
        key = ('b', M, N, K)
        return self._split.get(key) or fit_split(
            self._split, key, lambda: (lib.vitae_gemm_bf16x3_pick_split_k if self.prec == PREC['fp32x3'] else lib.vitae_gemm_pick_split_k)(M, N, K),
            lambda s: s * M * N, self.buf['ws'].numel())

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
            self._colsum(_ptr(dy), N, db, M, N)
        if dx is not None:
            lib.vitae_linear_bwd_input(self.prec, _ptr(dy), _ptr(self._param(wname)), _ptr(dx), M, N, K, epi, _ptr(aux), 0,
                                       self._split_bwd(M, K, N), ws, self.stream)

    def backward(self, kept, dfeat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """d loss / d features [B, D] -> {parameter name: gradient} for the trainable parameters of the encoder."""
        grads, dpool = self._backward_head(kept, dfeat)
        if dpool is None:
            return grads
        m = self.m
        B, L, D, H, P = kept['geom']
        N, M, depth, heads = L + 1, B * (L + 1), len(m.blocks), m.num_heads
        needs, f, st = kept['needs'], self._f, self.stream
        embed, lo = kept['embed'], kept['lo']
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


class HipEncoderTrainer16(_Trainer):
    """Fine-tuning on bf16 activations (``VisionTransformer3D(precision='bf16', activations='bf16')``): the kernels of the MAE engine's
    ``_block_fwd16`` / ``_block_bwd16`` (non-grouped form).  Every Linear runs on the LDS-DMA GEMM with bf16 operands written by their
    producers — LayerNorm's bf16 output, the qkv GEMM's bf16 q | k | v, the attention's ``o_16``, fc1's bf16 GELU and bf16 GELU' — and
    its backward is one paired launch (input gradient + weight gradient) whose dy operand the previous launch wrote in bf16.  Bias
    gradients ride on those launches (``dy_colsum`` / ``dx_colsum``).

    Kept per token row and block: x_in and xmid in fp32 (LayerNorm backward), o in fp32 (attention backward) and, in bf16, y1, q | k | v,
    o, y2, GELU' and the activation: 40 D bytes against 64 D, plus the row statistics.

    The weight-gradient half of a paired launch reduces over ``Mpad`` rows (M rounded up to 64) and needs rows M .. Mpad - 1 of both
    operands to be zero.  No such buffer outlives a call: each is allocated with ``Mpad`` rows in the call that fills it (``_z16``) and
    the pad rows of all of them are zeroed there by ONE multi-tensor launch in front of the call's first kernel (``_zero_pads``), so a
    smaller batch after a larger one finds nothing stale.  Frozen Linear: ``dw = NULL``, the
    launch computes the input gradient alone; its bias gradient then comes from a launch that does not depend on the weight
    gradient (fc1: the column sums of fc2's input-gradient epilogue; qkv: the attention backward's)."""

    ROUTE, SCRATCH, SCRATCH_ZEROED = 'bf16-activations', 'ws16', True
    act16 = True

    def __init__(self, module, precision: str = 'bf16'):
        super().__init__(module, precision)
        why = self._refusal(None)
        if why:
            raise VitaeError(why)
        self._pads = []

    def _refusal(self, in_chans):
        return act16_refusal_for(self.m, self.precision, in_chans)

    def _e16(self, *shape):
        return torch.empty(*shape, dtype=torch.bfloat16, device=self.device)

    def _z16(self, M, W):
        """A bf16 GEMM operand of M rows in a buffer of M rounded up to 64: the producers write rows < M only; the pad rows wait for
        ``_zero_pads``."""
        t = self._e16(_pad64(M), W)
        if t.shape[0] > M:
            self._pads.append(t[M:])
        return t

    def _zero_pads(self):
        """Zero the pad rows of every operand allocated since the last call, in one launch (a memset each was ~50 launches per ViT-B
        forward)."""
        if self._pads:
            torch._foreach_zero_(self._pads)
            self._pads = []

    def _patch_operand(self, T, P):
        return None, self._z16(T, P)

    def _block_bufs(self, B, N, D, H):
        """What one block keeps, except its input."""
        f, z, M = self._f, self._z16, B * N
        return {'mean1': f(M), 'rstd1': f(M), 'y1_16': z(M, D), 'qkv_16': self._e16(M, 3 * D), 'o': f(M, D), 'o_16': z(M, D),
                'lse': f(B * self.m.num_heads * N), 'xmid': f(M, D), 'mean2': f(M), 'rstd2': f(M), 'y2_16': z(M, D),
                'dgelu_16': self._e16(M, H), 'act_16': z(M, H)}

    def _block(self, q, k, x_in, x_out, B, N, D, H):
        self._block16(q, k, x_in, x_out, True, EPI_AUX_BF16 | EPI_AUX_DERIV, 'dgelu_16', B, N, D, H)

    # ------------------------------------------------------------------ backward
    def _pair(self, grads, needs, dy16, wname, x16, M, Mpad, N, K, dx=None, dx16=None, epi=EPI_NONE, aux=None, dx_colsum=None,
              dy_colsum=None):
        """Backward of y = x W^T + b on bf16 operands, dy16 [Mpad, N]: dx / dx16 [M, K] = epi(dy16 W16) and, for a trainable weight,
        dW = dy16^T x16 in the same launch.  ``dx_colsum`` / ``dy_colsum`` (zeroed by the caller) collect column sums of dx / dy16."""
        ws, key = self.buf['ws16'], ('p', M, N, K)
        s = self._split.get(key) or fit_split(
            self._split, key, lambda: lib.vitae_linear_bwd_pair_pick_split_k(M, Mpad, N, K), lambda s: lib.vitae_gemm_glds_ws_floats(M, K, s),
            ws.numel())
        dw = None
        if needs.get(wname):
            dw = grads[wname] = torch.empty_like(self._param(wname))
        assert dw is not None or dy_colsum is None      # the input-gradient-only form takes no column sums of dy16
        lib.vitae_linear_bwd_pair_glds(_ptr(dy16), self._bf16(wname), _ptr(x16), _ptr(dx), _ptr(dx16), _ptr(dw), None, M, Mpad, N, K,
                                       epi, _ptr(aux), _ptr(dx_colsum), _ptr(dy_colsum), 0, 0, s, ws.data_ptr(), ws.numel(), self.stream)

    def backward(self, kept, dfeat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """d loss / d features [B, D] -> {parameter name: gradient} for the trainable parameters of the encoder."""
        grads, dpool = self._backward_head(kept, dfeat)
        if dpool is None:
            return grads
        m = self.m
        B, L, D, H, P = kept['geom']
        N, M, depth, heads = L + 1, B * (L + 1), len(m.blocks), m.num_heads
        Mp = _pad64(M)
        needs, f, st = kept['needs'], self._f, self.stream
        embed, lo = kept['embed'], kept['lo']

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
        if depth > lo:
            dh16, dqkv16 = self._z16(M, H), self._z16(M, 3 * D)
            dy, do, delta = f(M, D), f(M, D), f(B * heads * N)
        dtok16 = self._z16(T, D) if (embed and needs.get('patch_embed.proj.weight')) else None
        self._zero_pads()
        for i in range(depth - 1, lo - 1, -1):
            q, k = f'blocks.{i}.', kept['blocks'][i]
            # fc1's bias gradient colsum(dh): beside fc1's weight gradient when there is one, else from fc2's input-gradient epilogue
            fc1_b = bias(q + 'mlp.fc1.bias')
            by_w = bool(needs.get(q + 'mlp.fc1.weight'))
            self._pair(grads, needs, dx16, q + 'mlp.fc2.weight', k['act_16'], M, Mp, D, H, dx16=dh16,
                       epi=EPI_DGELU | EPI_AUX_BF16 | EPI_AUX_DERIV, aux=k['dgelu_16'], dx_colsum=None if by_w else fc1_b)
            self._pair(grads, needs, dh16, q + 'mlp.fc1.weight', k['y2_16'], M, Mp, H, D, dx=dy, dy_colsum=fc1_b if by_w else None)
            self._ln_bwd(grads, needs, dy, k['xmid'], q + 'norm2.', k['mean2'], k['rstd2'], dx, M, D, 1, dx16, bias(q + 'attn.proj.bias'))
            self._pair(grads, needs, dx16, q + 'attn.proj.weight', k['o_16'], M, Mp, D, D, dx=do)
            # qkv's bias gradient colsum(dqkv): beside its weight gradient, or collected by the attention backward for a frozen weight
            qkv_b = bias(q + 'attn.qkv.bias')
            by_w = bool(needs.get(q + 'attn.qkv.weight'))
            lib.vitae_sdpa_mfma_bwd_bf16in(_ptr(k['qkv_16']), _ptr(k['o']), _ptr(do), _ptr(k['lse']), None, _ptr(dqkv16),
                                           None if by_w else _ptr(qkv_b), _ptr(delta), B, N, heads, self.hd, st)
            self._pair(grads, needs, dqkv16, q + 'attn.qkv.weight', k['y1_16'], M, Mp, 3 * D, D, dx=dy, dy_colsum=qkv_b if by_w else None)
            # norm1 leaves the output gradient of block i - 1: fp32, bf16, and its column sums = that block's fc2 bias gradient
            below = i > lo
            self._ln_bwd(grads, needs, dy, k['x_in'], q + 'norm1.', k['mean1'], k['rstd1'], dx, M, D, 1, dx16 if below else None,
                         bias(f'blocks.{i - 1}.mlp.fc2.bias') if below else None)
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
                self._colsum(dpos.data_ptr() + 4 * D, D, db, L, D)
            if want_w:
                # dW[D, P] = dtok16^T @ patches16 (both row-contiguous bf16, reduced over the padded token count)
                dw = grads['patch_embed.proj.weight'] = torch.empty_like(self._param('patch_embed.proj.weight'))
                lib.vitae_gemm_glds(0, 0, _ptr(dtok16), D, _ptr(kept['patches']), P, _ptr(dw), P, None, P, D, P, _pad64(T), None, None, 0,
                                    EPI_NONE, None, 0, 0, 1, None, None, st)
        return {n: g for n, g in grads.items() if g is not None}

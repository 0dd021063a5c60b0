"""MoCo v3 around ``VisionTransformer3D`` and around the 3-D ResNet (reference other_baselines/mocov3/moco/builder.py; Chen, Xie, He:
"An Empirical Study of Training Self-Supervised Vision Transformers", 2021): a base encoder and a momentum encoder with projector MLPs, a predictor MLP, the
symmetrised InfoNCE loss.  Names, signatures and state-dict keys are the reference's; the arithmetic runs on libvitae_hip.so:

  * ``MoCo_ViT``: the encoders go through ``forward_features`` once per step and encoder on the stacked views (trainer route for the
    base encoder, inference route for the momentum encoder);
  * ``MoCo_ResNet``: the two views go through the ResNet's launch sequence one after the other, so that every BatchNorm3d sees one
    view's batch statistics and its running statistics move twice per step, first view first — the body's autograd node once per view
    for the base encoder, ``forward_features(batch_stats=True)`` (batch statistics, nothing kept) for the momentum encoder;
  * the MLPs are autograd nodes over ``vitae_linear_*`` (no bias), ``vitae_bn1d_relu_*`` and ``vitae_bn1d_*``, one view at a time, so
    BatchNorm statistics are per view and running statistics move twice per step, first view first;
  * ``_update_momentum_encoder`` is ``vitae_ema_multi`` (one launch for all parameters), ``contrastive_loss`` / the loss of ``forward`` is
    ``vitae_moco_loss`` (three launches, both terms and their gradients).

There is no CPU fallback: a CPU input raises ``VitaeError``.  Not built: ``concat_all_gather`` / several GPUs, SyncBatchNorm, the
Bottleneck depths of the ResNet (50 - 200).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ...._abi import VitaeError, lib
from ....k_fold_training_scripts.resnet_3d import ResNet as _PackageResNet
from ....model.vit import _stream, hip_linear
from ....shadow import mark_current, shadow_column
from .optimizer import TableRing, ema_table, fp32_on_device


class _LinearNoBias(torch.autograd.Function):
    """``y = x W^T`` on the HIP GEMM launchers, forward and backward (fp32 operands; the MLPs' GEMMs have 2 to 64 rows)."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous().float()
        if x.shape[1] % 4 or weight.shape[0] % 4:
            raise VitaeError(f'MoCo MLP: Linear sizes must be multiples of 4 (got {tuple(weight.shape)})')
        fp32_on_device(weight, 'MoCo MLP: a Linear weight')
        ctx.save_for_backward(x, weight)
        return hip_linear(x, weight, None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        (M, K), N = x.shape, weight.shape[0]
        dy = dy.contiguous().float()
        st = _stream(x)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            lib.vitae_linear_bwd_input(0, dy.data_ptr(), weight.data_ptr(), dx.data_ptr(), M, N, K, 0, None, 0, 1, None, st)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            lib.vitae_linear_bwd_weight(0, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), M, N, K, 0, 1, None, st)
        return dx, dw


class _BatchNorm(torch.autograd.Function):
    """``nn.BatchNorm1d`` (+ ReLU when ``relu``) in training mode: batch statistics, running statistics updated in place."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu):
        x = x.contiguous().float()
        R, D = x.shape
        if bn.momentum is None:
            raise VitaeError('BatchNorm1d(momentum=None) (cumulative average) is not supported')
        y = torch.empty_like(x)
        mean = torch.empty(D, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        rm, rv, nbt = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if bn.track_running_stats else (None, None, None)
        for t in (weight, bias, rm, rv):
            if t is not None:
                fp32_on_device(t, 'MoCo MLP: a BatchNorm tensor')
        p = lambda t: None if t is None else t.data_ptr()
        if relu:
            lib.vitae_bn1d_relu_fwd(x.data_ptr(), p(weight), p(bias), y.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(), p(rm), p(rv), p(nbt),
                                    R, D, bn.eps, bn.momentum, _stream(x))
        else:
            lib.vitae_bn1d_fwd(x.data_ptr(), p(weight), p(bias), y.data_ptr(), None, mean.data_ptr(), rstd.data_ptr(), p(rm), p(rv), p(nbt),
                               R, D, bn.eps, bn.momentum, _stream(x))
        ctx.relu, ctx.affine = relu, weight is not None
        ctx.save_for_backward(x, y if relu else None, weight, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, weight, mean, rstd = ctx.saved_tensors
        R, D = x.shape
        dy = dy.contiguous().float()
        dx = torch.empty_like(x)
        dw = db = None
        if ctx.affine:                       # the launchers add their column sums
            dw, db = torch.zeros_like(weight), torch.zeros_like(weight)
        p = lambda t: None if t is None else t.data_ptr()
        if ctx.relu:
            lib.vitae_bn1d_relu_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    dx.data_ptr(), None, dw.data_ptr(), db.data_ptr(), R, D, _stream(x))
        else:
            lib.vitae_bn1d_bwd(dy.data_ptr(), x.data_ptr(), p(weight), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), None, p(dw), p(db),
                               R, D, _stream(x))
        return dx, dw, db, None, None


def _batchnorm_eval(x, bn, relu):
    x = x.contiguous().float()
    R, D = x.shape
    if not bn.track_running_stats:
        raise VitaeError('BatchNorm1d without running statistics has no eval form')
    y = torch.empty_like(x)
    p = lambda t: None if t is None else t.data_ptr()
    fn = lib.vitae_bn1d_relu_eval if relu else lib.vitae_bn1d_eval
    fn(x.data_ptr(), p(bn.weight), p(bn.bias), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), y.data_ptr(), R, D, bn.eps, _stream(x))
    return y


def run_mlp(mlp: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """One of the MLPs ``MoCo._build_mlp`` makes, on the HIP launchers: Linear(bias=False), BatchNorm1d [+ ReLU], ...  In ``eval()`` mode
    (or for a BatchNorm in it) the running statistics normalise and nothing is differentiated."""
    mods = list(mlp)
    i = 0
    while i < len(mods):
        mod = mods[i]
        if isinstance(mod, nn.Linear):
            if mod.bias is not None:
                raise VitaeError('MoCo MLP: Linear layers carry no bias')
            x = _LinearNoBias.apply(x, mod.weight)
        elif isinstance(mod, nn.BatchNorm1d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            if relu and mod.weight is None:
                raise VitaeError('MoCo MLP: BatchNorm1d(affine=False) followed by ReLU is not built')
            if mod.training:
                x = _BatchNorm.apply(x, mod.weight, mod.bias, mod, relu)
            else:
                if torch.is_grad_enabled() and x.requires_grad:
                    raise VitaeError('MoCo MLP: BatchNorm1d in eval() mode has no backward; call the model under torch.no_grad()')
                x = _batchnorm_eval(x, mod, relu)
            i += relu
        else:
            raise VitaeError(f'MoCo MLP: {type(mod).__name__} is not part of the MLPs this package builds')
        i += 1
    return x


class _MocoLoss(torch.autograd.Function):
    """``contrastive_loss(q1, k2) + contrastive_loss(q2, k1)`` and both query gradients from one ``vitae_moco_loss`` call; the backward
    scales the stored gradients by the incoming one on the device."""

    @staticmethod
    def forward(ctx, q1, k2, q2, k1, T):
        ts = [t.detach().contiguous().float() for t in (q1, k2, q2, k1)]
        N, C = ts[0].shape
        for t in ts:
            if not t.is_cuda:
                raise VitaeError(f'contrastive_loss: input is on {t.device}; this package computes on MI355X only (no CPU fallback)')
            if t.shape != (N, C) or t.device != ts[0].device:
                raise VitaeError('contrastive_loss: queries and keys must be [N, C] tensors of one shape on one device')
        dev = ts[0].device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dq1, dq2 = torch.empty_like(ts[0]), torch.empty_like(ts[2])
        ws = torch.empty(max(4, int(lib.vitae_moco_loss_ws_floats(N, C))), dtype=torch.float32, device=dev)
        lib.vitae_moco_loss(*(t.data_ptr() for t in ts), N, C, float(T), loss.data_ptr(), dq1.data_ptr(), dq2.data_ptr(), ws.data_ptr(),
                            _stream(ts[0]))
        ctx.save_for_backward(dq1, dq2)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dq1, dq2 = ctx.saved_tensors
        return (dq1 * g if ctx.needs_input_grad[0] else None, None, dq2 * g if ctx.needs_input_grad[2] else None, None, None)


class MoCo(nn.Module):
    """A base encoder, a momentum encoder (a copy that follows it by an exponential moving average and gets no gradient), a projector
    MLP on each as their ``head`` and a predictor MLP.  ``base_encoder``: a callable taking ``num_classes=``, in practice
    ``partial(VisionTransformer3D, in_chans=..., volume_size=..., [precision=..., activations=...])``.  ``dim``: output size of the
    MLPs, ``mlp_dim``: their hidden size, ``T``: softmax temperature."""

    # (name of the encoder attribute that becomes its projector, projector layers, predictor layers): set by the subclass
    PROJECTOR_ATTR, PROJECTOR_LAYERS, PREDICTOR_LAYERS = None, 0, 0

    def __init__(self, base_encoder, dim=256, mlp_dim=4096, T=1.0):
        super().__init__()
        self.T = T
        for name in ('base_encoder', 'momentum_encoder'):
            setattr(self, name, self._checked_encoder(base_encoder(num_classes=mlp_dim)))
        self._build_projector_and_predictor_mlps(dim, mlp_dim)
        # the momentum encoder starts as the base encoder, projector included, and is never stepped by an optimiser
        self.momentum_encoder.load_state_dict(self.base_encoder.state_dict())
        self.momentum_encoder.requires_grad_(False)
        self._ema_ring = TableRing()
        self._configure_encoders()

    def _checked_encoder(self, encoder):
        """What ``base_encoder(...)`` returned, or the subclass's refusal of it (before anything is attached or replaced)."""
        return encoder

    def _configure_encoders(self):
        # LayerNorm parameter gradients (encoder._Trainer._ln_bwd) and, on the fp32-activation routes, Linear bias gradients (_colsum)
        # of the trained encoder without atomics: sums that cancel reproduce from run to run, and a loss scaled by a power of two
        # (GradScaler) gives the unscaled run's gradients.  (An embedding size those forms do not serve raises in the backward.)
        self.base_encoder.ordered_norm_grads = True

    def _build_mlp(self, num_layers, input_dim, mlp_dim, output_dim, last_bn=True):
        """``num_layers`` bias-free Linear layers input_dim -> mlp_dim -> ... -> output_dim; BatchNorm1d + ReLU between them, and a
        BatchNorm1d without scale and shift after the last one when ``last_bn``."""
        layers = []
        for i in range(num_layers):
            last = i == num_layers - 1
            d_in, d_out = (mlp_dim if i else input_dim), (output_dim if last else mlp_dim)
            layers.append(nn.Linear(d_in, d_out, bias=False))
            if not last:
                layers += [nn.BatchNorm1d(d_out), nn.ReLU(inplace=True)]
            elif last_bn:
                layers.append(nn.BatchNorm1d(d_out, affine=False))
        return nn.Sequential(*layers)

    def _build_projector_and_predictor_mlps(self, dim, mlp_dim):
        """Put a projector in place of each encoder's classifier and make the predictor, from the subclass's layer counts."""
        if self.PROJECTOR_ATTR is None:
            return
        width = self.base_encoder.embed_dim                 # the encoders' feature size
        for enc in (self.base_encoder, self.momentum_encoder):
            setattr(enc, self.PROJECTOR_ATTR, self._build_mlp(self.PROJECTOR_LAYERS, width, mlp_dim, dim))
        self.predictor = self._build_mlp(self.PREDICTOR_LAYERS, dim, mlp_dim, dim)

    @torch.no_grad()
    def _update_momentum_encoder(self, m):
        """``pm <- pm * m + pb * (1. - m)`` for every parameter pair, in one launch (the statement's fp32 arithmetic, bit for bit)."""
        pairs = [(pb, pm) for pb, pm in zip(self.base_encoder.parameters(), self.momentum_encoder.parameters()) if pm.numel()]
        if not pairs:
            return
        device = pairs[0][1].device
        for pb, pm in pairs:
            fp32_on_device(pb, '_update_momentum_encoder: a base parameter')
            fp32_on_device(pm, '_update_momentum_encoder: a momentum parameter')
            if pb.shape != pm.shape or pb.device != device or pm.device != device:
                raise VitaeError('_update_momentum_encoder: the two encoders must hold the same parameters on one device')
        lengths = [pm.numel() for _, pm in pairs]
        table = ema_table([pm.data_ptr() for _, pm in pairs], [pb.data_ptr() for pb, _ in pairs], lengths)
        # bf16 slots of the momentum encoder that hold its weights as they are now get the new ones in the same pass (shadow.py)
        column, listed = shadow_column([pm for _, pm in pairs])
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream()
            a = self._ema_ring.send(device, table, lengths, shadow=column)
            if a['sh'] is None:
                lib.vitae_ema_multi(a['th'], a['td'], a['nt'], a['ch'], a['cd'], a['nc'], a['chunk'], float(m), stream.cuda_stream)
            else:
                lib.vitae_ema_multi_shadow(a['th'], a['td'], a['nt'], a['ch'], a['cd'], a['nc'], a['chunk'], float(m), a['sh'], a['sd'],
                                           stream.cuda_stream)
            self._ema_ring.done(a['slot'], stream)
        # written through raw pointers: whatever is keyed on p._version must see it; the listed slots hold the new version
        torch.autograd.graph.increment_version([pm for _, pm in pairs])
        mark_current(listed)

    def contrastive_loss(self, q, k):
        """InfoNCE of one (query, key) pair: rows normalised, logits q k^T / T, cross-entropy against the diagonal, times 2 T."""
        # the launcher computes two terms at once; given the same pair twice it returns twice this one, and the two (equal) query
        # gradients sum to twice this one's: halving both is exact
        return _MocoLoss.apply(q, k, q, k, self.T) * 0.5

    def _views(self, x1, x2):
        """What ``_features`` takes: here the stacked views, one encoder call for both (the encoder has no batch statistics)."""
        return torch.cat([x1, x2], dim=0)

    def _features(self, encoder, views, momentum):
        """-> the encoder's features of the first and of the second view.  ``momentum``: this is the momentum encoder, under no_grad."""
        f = encoder.forward_features(views)
        B = f.shape[0] // 2
        return f[:B], f[B:]

    def _heads(self, encoder, f1, f2):
        """The projector of ``encoder`` on each view's features, first view first."""
        mlp = getattr(encoder, self.PROJECTOR_ATTR)
        return run_mlp(mlp, f1), run_mlp(mlp, f2)

    def forward(self, x1, x2, m):
        """x1, x2: the two views [B, C, L, H, W]; m: momentum of the update.  -> the loss (0-dim; differentiable in training mode)."""
        for x in (x1, x2):
            if not x.is_cuda:
                raise VitaeError(f'MoCo.forward: input is on {x.device}; this package computes on MI355X only (no CPU fallback)')
        if x1.shape != x2.shape:
            raise VitaeError('MoCo.forward: the two views must have one shape')
        x = self._views(x1, x2)
        # the encoder as the subclass runs it (_features); heads and predictor per view
        # (eval() mode is inference, as for VisionTransformer3D: running statistics normalise, nothing is differentiated)
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.training):
            p1, p2 = self._heads(self.base_encoder, *self._features(self.base_encoder, x, False))
            q1, q2 = run_mlp(self.predictor, p1), run_mlp(self.predictor, p2)
        with torch.no_grad():
            self._update_momentum_encoder(m)
            k1, k2 = self._heads(self.momentum_encoder, *self._features(self.momentum_encoder, x, True))
        return _MocoLoss.apply(q1, k2, q2, k1, self.T)


class MoCo_ResNet(MoCo):
    """MoCo v3 over this package's 3-D ResNet (``resent3d_base.generate_model`` / ``k_fold_training_scripts.resnet_3d``; depths 10 / 18
    / 34): a 2-layer projector in place of each encoder's ``fc``, a 2-layer predictor without a last BatchNorm.  ``base_encoder``: a
    callable taking ``num_classes=``, in practice ``partial(generate_model, model_depth=10, n_input_channels=...)``; one that returns
    anything but this package's ``ResNet`` is refused with ``NotImplementedError``."""
    PROJECTOR_ATTR = 'fc'

    def _checked_encoder(self, encoder):
        if not isinstance(encoder, _PackageResNet):
            raise NotImplementedError(f'MoCo_ResNet wraps only the 3-D ResNet of this package (resent3d_base.generate_model, depths 10 / 18 / '
                                      f'34), not {type(encoder).__module__}.{type(encoder).__qualname__}; MoCo_ViT wraps VisionTransformer3D')
        return encoder

    def _configure_encoders(self):
        pass                # the ResNet's backward has no atomics: nothing to switch

    def _build_projector_and_predictor_mlps(self, dim, mlp_dim):
        hidden_dim = self.base_encoder.fc.weight.shape[1]
        del self.base_encoder.fc, self.momentum_encoder.fc              # the classifiers
        self.base_encoder.fc = self._build_mlp(2, hidden_dim, mlp_dim, dim)
        self.momentum_encoder.fc = self._build_mlp(2, hidden_dim, mlp_dim, dim)
        self.predictor = self._build_mlp(2, dim, mlp_dim, dim, False)

    def _views(self, x1, x2):
        return x1, x2

    def _features(self, encoder, views, momentum):
        # one launch sequence per view, first view first: per-view batch statistics, running statistics moved twice.  The momentum
        # encoder stays in train() mode under no_grad in the reference: batch statistics there too (eval(): the running ones)
        batch_stats = True if momentum and encoder.training else None
        return tuple(encoder.forward_features(x, batch_stats=batch_stats) for x in views)


class MoCo_ViT(MoCo):
    """MoCo v3 over ``VisionTransformer3D``: a 3-layer projector as each encoder's ``head``, a 2-layer predictor."""
    PROJECTOR_ATTR, PROJECTOR_LAYERS, PREDICTOR_LAYERS = 'head', 3, 2

"""Batch-mode Mixup for the fine-tuning loop (reference post_training_utils/fine_tune_epoch.py:31,58-59,366-369:
``Mixup(mixup_alpha=0.1, num_classes=2)`` from ``timm.data.mixup``, passed to ``train_one_epoch`` as ``mix_up_fn``).

``timm`` is not a dependency of this package and was not available when this was written: the constructor signature, the order
of the random draws and the label-smoothing formula below restate timm's documented batch mode, and parity with timm itself
is UNPINNED (no fixture records its outputs) — as for the ``torchio`` augmentations of ``utils/augment.py``.

    lam    : ``np.random.rand() < prob`` first, then ``np.random.beta(mixup_alpha, mixup_alpha)`` — both from the global numpy
             stream, so a script's ``np.random.seed`` means what it meant; 1.0 when the first draw says no
    x      : ``x <- lam x + (1 - lam) x.flip(0)``, in place, by ``vitae_mixup_pairs`` (one read and one write of the batch)
    target : ``lam onehot(y) + (1 - lam) onehot(y.flip(0))`` with ``onehot`` smoothed to ``label_smoothing / num_classes`` off
             and ``1 - label_smoothing + label_smoothing / num_classes`` on the class, by ``vitae_mixup_targets``

Deviations: an odd batch is served (timm asserts an even one; the middle sample is mixed with itself, i.e. left as it is);
CutMix (``cutmix_alpha > 0``, ``cutmix_minmax``) and the ``'elem'`` / ``'pair'`` modes are not built and raise
``NotImplementedError``.  ``switch_prob`` and ``correct_lam`` only matter to CutMix and are accepted for the signature.
"""
import numpy as np
import torch

from .._abi import VitaeError, lib


class Mixup:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        if cutmix_alpha > 0. or cutmix_minmax is not None:
            raise NotImplementedError('CutMix (cutmix_alpha > 0, cutmix_minmax) is not built for MI355X')
        if mode != 'batch':
            raise NotImplementedError(f"Mixup mode {mode!r} is not built for MI355X (only 'batch')")
        if not mixup_alpha > 0.:
            raise ValueError('mixup_alpha must be > 0 (CutMix, the other source of a mixing ratio, is not built)')
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        self.mix_prob, self.switch_prob = prob, switch_prob
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mode, self.correct_lam = mode, correct_lam
        self.mixup_enabled = True       # as timm: set to False to pass batches through with lam = 1
        self.last_lam = None            # the ratio of the latest call

    def _params_per_batch(self):
        lam = 1.
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            lam = float(np.random.beta(self.mixup_alpha, self.mixup_alpha))
        return lam

    def __call__(self, x, target):
        if not x.is_cuda or not target.is_cuda:
            raise VitaeError(f'Mixup: the batch is on {x.device}, the labels on {target.device}; this package computes on MI355X '
                             f'only (no CPU fallback).')
        B = x.shape[0]
        if target.dim() != 1 or target.shape[0] != B or target.dtype != torch.int64:
            raise ValueError(f'Mixup: labels must be int64 of shape ({B},), got {target.dtype} {tuple(target.shape)}')
        lam = self.last_lam = self._params_per_batch()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()           # a copy is mixed instead of the caller's tensor
        st = torch.cuda.current_stream(x.device).cuda_stream
        lib.vitae_mixup_pairs(x.data_ptr(), None, lam, B, x.numel() // B, st)
        out = torch.empty(B, self.num_classes, dtype=torch.float32, device=x.device)
        lib.vitae_mixup_targets(target.contiguous().data_ptr(), out.data_ptr(), lam, float(self.label_smoothing), B,
                                self.num_classes, st)
        return x, out

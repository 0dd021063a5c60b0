"""Class-weighted soft-target cross entropy (reference: utils/custom_loss.py:7-18).

Only used by the reference's mix-up fine-tuning scripts, never by the pre-training hot path
(the masked reconstruction loss lives in model/vit_autoenc.py:205-232).  Kept as a small
plain-torch module so ``from utils.custom_loss import SoftCrossEntropyWithWeightsLoss`` resolves.

``HipSoftCrossEntropyWithWeightsLoss`` is the same criterion, and ``HipCrossEntropyLoss`` is
``torch.nn.CrossEntropyLoss(weight=...)`` (mean reduction, ignore_index -100: the other criterion of the fine-tuning script,
post_training_utils/fine_tune_epoch.py:366-376), each as ONE launch of ``vitae_cls_loss`` (csrc/classify.hip) behind one
autograd node instead of a string of small elementwise launches.  They compute on the device only.
"""
import torch
from torch import nn

from .._abi import VitaeError, lib


class SoftCrossEntropyWithWeightsLoss(nn.Module):
    def __init__(self, weights):
        super().__init__()
        self.weights = nn.Parameter(torch.as_tensor(weights), requires_grad=False)

    def forward(self, y_hat, y):
        # per class c: sum_n -y[n,c] * w[c] * log_softmax(y_hat)[n,c] / sum(w); then mean over classes
        logp = torch.log_softmax(y_hat, dim=-1)
        per_class = (-(y * logp) * self.weights).sum(dim=0) / self.weights.sum()
        return per_class.mean()

    def __repr__(self):
        return f"weights are on {self.weights.device}\n"


class _ClsLossFunction(torch.autograd.Function):
    """``apply(logits [B, C], target, weight or None, hard) -> loss``: the forward's one launch leaves the loss and the
    gradient of the logits for an upstream gradient of 1; the backward multiplies it by the incoming scalar."""

    @staticmethod
    def forward(ctx, logits, target, weight, hard):
        x = logits.detach()
        if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.float().contiguous()
        B, C = x.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dl = torch.empty(B, C, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None
        lib.vitae_cls_loss(x.data_ptr(), x.stride(0), target.data_ptr() if hard else None, None if hard else target.data_ptr(),
                           None if weight is None else weight.data_ptr(), 1.0, loss.data_ptr(),
                           None if dl is None else dl.data_ptr(), None, None, None, B, C,
                           torch.cuda.current_stream(x.device).cuda_stream)
        ctx.dl, ctx.released = dl, False
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        if ctx.released:
            raise VitaeError('vitae_cls_loss: backward called twice on one forward (the gradient is released after the first)')
        dl, ctx.dl, ctx.released = ctx.dl, None, True
        return (None if dl is None else dl.mul_(gout)), None, None, None


def _cls_loss(what, logits, target, weight, hard):
    if not logits.is_cuda or not target.is_cuda:
        raise VitaeError(f'{what}: logits are on {logits.device}, targets on {target.device}; this package computes on MI355X '
                         f'only (no CPU fallback).')
    if logits.dim() != 2:
        raise ValueError(f'{what}: logits must be [batch, classes], got {tuple(logits.shape)}')
    B, C = logits.shape
    if hard:
        if target.dtype != torch.int64 or tuple(target.shape) != (B,):
            raise ValueError(f'{what}: class indices must be int64 of shape ({B},), got {target.dtype} {tuple(target.shape)}')
    elif tuple(target.shape) != (B, C):
        raise ValueError(f'{what}: soft targets must have the shape of the logits {(B, C)}, got {tuple(target.shape)}')
    target = target.detach().contiguous() if hard else target.detach().float().contiguous()
    if weight is not None:
        if weight.numel() != C or weight.device != logits.device:
            raise ValueError(f'{what}: {weight.numel()} class weights on {weight.device} for {C} classes on {logits.device}')
        weight = weight.detach().float().contiguous()
    return _ClsLossFunction.apply(logits, target, weight, hard)


class HipCrossEntropyLoss(nn.Module):
    """``torch.nn.CrossEntropyLoss(weight=weight)`` on class indices (mean reduction, ignore_index -100)."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer('weight', None if weight is None else torch.as_tensor(weight).detach().clone().float())

    def forward(self, input, target):
        return _cls_loss('HipCrossEntropyLoss', input, target, self.weight, True)


class HipSoftCrossEntropyWithWeightsLoss(nn.Module):
    """``SoftCrossEntropyWithWeightsLoss`` above; same constructor, same value."""

    def __init__(self, weights):
        super().__init__()
        self.weights = nn.Parameter(torch.as_tensor(weights).detach().clone().float(), requires_grad=False)

    def forward(self, y_hat, y):
        return _cls_loss('HipSoftCrossEntropyWithWeightsLoss', y_hat, y, self.weights, False)

    def __repr__(self):
        return f"weights are on {self.weights.device}\n"

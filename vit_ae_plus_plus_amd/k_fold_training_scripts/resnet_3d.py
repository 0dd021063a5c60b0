"""The supervised 3-D ResNet baseline (reference k_fold_training_scripts/resnet_3d.py) on the HIP kernels of csrc/conv3d.hip.

Same constructor arguments, attribute names, state-dict keys and shapes (``conv1.weight``, ``bn1.*``, ``layerK.i.conv1.weight``,
``layerK.0.downsample.0.weight``, ``layerK.0.downsample.1.*``, ``fc.*``) and the same initialisation (Kaiming-normal ``fan_out`` for the
convolutions, 1 / 0 for BatchNorm), so checkpoints interchange.  Parameters are ordinary fp32 ``nn.Parameter``s in torch layout;
``torch.optim.Adam(model.parameters(), lr)`` and ``NativeScalerWithGradNormCount`` work unchanged.

The sub-modules only HOLD parameters and buffers: the arithmetic runs in ``ResNet.forward`` through ``vit_ae_plus_plus_amd.resnet``
(one autograd node for the body, one for the head in ``train()`` mode with gradients enabled; inference on the running statistics in
``eval()`` mode or under ``no_grad``; ``forward_features`` is the same below ``fc``, and with ``batch_stats=True`` under ``no_grad`` the
training arithmetic with nothing kept: a MoCo momentum encoder).  Calling a sub-module on its own raises ``VitaeError`` — there is no
torch fallback.  Operands of the convolutions and of the head are bf16 with fp32 accumulation: the counterpart of the reference
script's autocast region.  ``precision='fp32x3'`` (keyword-only; ``set_precision`` later) is the parity-grade route: every fp32 operand
of the convolutions and of the head enters the bf16 MFMA as hi + lo halves (three products), ~1e-5 from a float64 run instead of
percent.  An exact-fp32 convolution is not built: any other value raises ``VitaeError``.

Served: depths 10 / 18 / 34 (BasicBlock), shortcut 'B', any ``widen_factor`` whose widths stay multiples of 4.
Refused at construction (``NotImplementedError``): depths 50 - 200 (Bottleneck) and shortcut 'A'.
"""
import torch
import torch.nn as nn

from .._abi import CONSTS, VitaeError
from ..model.vit import _HeadFunction, hip_linear
from ..resnet import HipResNetRunner, check_precision


def get_inplanes():
    return [64, 128, 256, 512]


class _HoldsParameters:
    """Mixed into the torch layer classes below: same parameters, buffers and ``isinstance`` answers, no stand-alone forward."""

    def forward(self, *a, **k):
        raise VitaeError(f'{type(self).__name__}: the layers of the 3-D ResNet run only inside ResNet.forward (HIP launch sequence); '
                         f'there is no stand-alone module forward and no torch fallback')


class Conv3d(_HoldsParameters, nn.Conv3d):
    pass


class BatchNorm3d(_HoldsParameters, nn.BatchNorm3d):
    pass


class MaxPool3d(_HoldsParameters, nn.MaxPool3d):
    pass


def conv3x3x3(in_planes, out_planes, stride=1):
    return Conv3d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


def conv1x1x1(in_planes, out_planes, stride=1):
    return Conv3d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class BasicBlock(_HoldsParameters, nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3x3(in_planes, planes, stride)
        self.bn1 = BatchNorm3d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3x3(planes, planes)
        self.bn2 = BatchNorm3d(planes)
        self.downsample = downsample
        self.stride = stride


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, *a, **k):
        raise NotImplementedError('Bottleneck (depths 50 - 200) is not built for MI355X; depths 10 / 18 / 34 are')


class _BodyFunction(torch.autograd.Function):
    """``apply(runner, names, x, *params) -> features [N, C]``: everything below the head as one autograd node.  Forward keeps the
    activations on the context; backward returns one gradient per parameter and none for the input volume."""

    @staticmethod
    def forward(ctx, runner, names, x, *params):
        feat, kept = runner.forward_keep(x)
        ctx.runner, ctx.names, ctx.kept = runner, names, kept
        return feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dfeat):
        if ctx.kept is None:
            raise VitaeError('ResNet: backward called twice on one forward (activations are released after the first)')
        grads = ctx.runner.backward(ctx.kept, dfeat)
        ctx.kept = None
        return (None, None, None) + tuple(grads[n] if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[3:]))


class ResNet(nn.Module):

    def __init__(self, block, layers, block_inplanes, n_input_channels=3, conv1_t_size=7, conv1_t_stride=1, no_max_pool=False,
                 shortcut_type='B', widen_factor=1.0, n_classes=400, *, precision='bf16'):
        super().__init__()
        self.precision = check_precision(precision)
        if block is not BasicBlock:
            raise NotImplementedError('only BasicBlock networks (depths 10 / 18 / 34) are built for MI355X')
        if shortcut_type != 'B':
            raise NotImplementedError("only shortcut_type 'B' (1x1x1 convolution + BatchNorm) is built for MI355X")
        block_inplanes = [int(x * widen_factor) for x in block_inplanes]
        if any(w <= 0 or w % 4 for w in block_inplanes):
            raise NotImplementedError(f'channel widths {block_inplanes} must be positive multiples of 4')
        if not (1 <= conv1_t_size <= 7 and conv1_t_stride in (1, 2)):
            raise NotImplementedError('conv1_t_size must be 1..7 and conv1_t_stride 1 or 2')

        self.in_planes = block_inplanes[0]
        self.no_max_pool = no_max_pool
        self.conv1 = Conv3d(n_input_channels, self.in_planes, kernel_size=(conv1_t_size, 7, 7), stride=(conv1_t_stride, 2, 2),
                            padding=(conv1_t_size // 2, 3, 3), bias=False)
        self.bn1 = BatchNorm3d(self.in_planes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = MaxPool3d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, block_inplanes[0], layers[0], shortcut_type)
        self.layer2 = self._make_layer(block, block_inplanes[1], layers[1], shortcut_type, stride=2)
        self.layer3 = self._make_layer(block, block_inplanes[2], layers[2], shortcut_type, stride=2)
        self.layer4 = self._make_layer(block, block_inplanes[3], layers[3], shortcut_type, stride=2)
        self.avgpool = nn.AdaptiveAvgPool3d((1, 1, 1))
        self.fc = nn.Linear(block_inplanes[3] * block.expansion, n_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm3d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, shortcut_type, stride=1):
        downsample = None
        if stride != 1 or self.in_planes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1x1(self.in_planes, planes * block.expansion, stride), BatchNorm3d(planes * block.expansion))
        layers = [block(in_planes=self.in_planes, planes=planes, stride=stride, downsample=downsample)]
        self.in_planes = planes * block.expansion
        layers += [block(self.in_planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward_features(self, x, *, batch_stats=None):
        """Everything below ``fc``: the pooled features ``[N, C]``.

        ``batch_stats=None``: the rule of ``forward`` — the body's autograd node in ``train()`` mode with gradients enabled, inference on
        the running statistics otherwise.  ``batch_stats=True`` (``train()`` mode under ``torch.no_grad()`` only, ``VitaeError`` otherwise):
        BatchNorm on batch statistics with the running statistics and ``num_batches_tracked`` updated, nothing kept for a backward —
        what a MoCo momentum encoder computes."""
        runner = HipResNetRunner(self)
        if batch_stats:
            if torch.is_grad_enabled() or not self.training:
                raise VitaeError('ResNet.forward_features(batch_stats=True) keeps nothing for a backward and updates the running statistics: '
                                 'call it in train() mode under torch.no_grad()')
            return runner.forward_batch_stats(x)
        if self.training and torch.is_grad_enabled():
            body = [(n, p) for n, p in self.named_parameters() if not n.startswith('fc.')]
            return _BodyFunction.apply(runner, tuple(n for n, _ in body), x, *(p for _, p in body))
        with torch.no_grad():
            return runner.infer(x)

    def set_precision(self, precision):
        """``'bf16'`` | ``'fp32x3'`` from the next forward on (anything else: ``VitaeError``).  The packed operands of the other route
        are dropped when the new one first asks for its own."""
        self.precision = check_precision(precision)
        return self

    def forward(self, x):
        prec = CONSTS['VITAE_PREC_BF16X3' if check_precision(self.precision) == 'fp32x3' else 'VITAE_PREC_BF16']
        feat = self.forward_features(x)
        if self.training and torch.is_grad_enabled():
            return _HeadFunction.apply(feat, self.fc.weight, self.fc.bias, prec)
        with torch.no_grad():
            return hip_linear(feat, self.fc.weight, self.fc.bias, precision=prec)


def generate_model(model_depth, **kwargs):
    assert model_depth in [10, 18, 34, 50, 101, 152, 200]
    layers = {10: [1, 1, 1, 1], 18: [2, 2, 2, 2], 34: [3, 4, 6, 3]}.get(model_depth)
    if layers is None:
        raise NotImplementedError(f'depth {model_depth} is a Bottleneck network: not built for MI355X (depths 10 / 18 / 34 are)')
    return ResNet(BasicBlock, layers, get_inplanes(), **kwargs)

"""The MoCo v3 baseline's copy of the 3-D ResNet (reference other_baselines/mocov3/moco/resent3d_base.py).  It differs from
``k_fold_training_scripts/resnet_3d.py`` in one keyword, ``num_classes`` for ``n_classes``; everything else here IS that module:
same layer classes, state-dict keys, shapes, initialisation, refusals (Bottleneck depths, shortcut 'A') and the same HIP launch
sequence (``vit_ae_plus_plus_amd.resnet``).  ``builder.MoCo_ResNet`` wraps what ``generate_model`` of this module makes.
"""
from ....k_fold_training_scripts import resnet_3d as _base
from ....k_fold_training_scripts.resnet_3d import BasicBlock, Bottleneck, conv1x1x1, conv3x3x3, get_inplanes  # noqa: F401


class ResNet(_base.ResNet):

    def __init__(self, block, layers, block_inplanes, n_input_channels=3, conv1_t_size=7, conv1_t_stride=1, no_max_pool=False,
                 shortcut_type='B', widen_factor=1.0, num_classes=400, *, precision='bf16'):
        super().__init__(block, layers, block_inplanes, n_input_channels=n_input_channels, conv1_t_size=conv1_t_size,
                         conv1_t_stride=conv1_t_stride, no_max_pool=no_max_pool, shortcut_type=shortcut_type, widen_factor=widen_factor,
                         n_classes=num_classes, precision=precision)


def generate_model(model_depth, **kwargs):
    assert model_depth in [10, 18, 34, 50, 101, 152, 200]
    layers = {10: [1, 1, 1, 1], 18: [2, 2, 2, 2], 34: [3, 4, 6, 3]}.get(model_depth)
    if layers is None:
        raise NotImplementedError(f'depth {model_depth} is a Bottleneck network: not built for MI355X (depths 10 / 18 / 34 are)')
    return ResNet(BasicBlock, layers, get_inplanes(), **kwargs)

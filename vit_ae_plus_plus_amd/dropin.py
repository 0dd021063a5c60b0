"""Make ``import model...`` / ``import utils...`` (the reference's top-level package names,
e.g. ``from model.model_factory import get_models``, ``from utils import misc, lr_sched`` in
k_fold_training_scripts/k_fold_cross_valid_combined_brats.py) resolve to this package.

    import vit_ae_plus_plus_amd.dropin; vit_ae_plus_plus_amd.dropin.install()
    # ... then run the reference's pre-training script unchanged
"""
import importlib
import sys

_ALIASES = {
    'model': 'vit_ae_plus_plus_amd.model',
    'model.model_factory': 'vit_ae_plus_plus_amd.model.model_factory',
    'model.vit': 'vit_ae_plus_plus_amd.model.vit',
    'model.vit_autoenc': 'vit_ae_plus_plus_amd.model.vit_autoenc',
    'model.model_utils': 'vit_ae_plus_plus_amd.model.model_utils',
    'model.model_utils.vit_helpers': 'vit_ae_plus_plus_amd.model.model_utils.vit_helpers',
    'model.model_utils.sobel_filter': 'vit_ae_plus_plus_amd.model.model_utils.sobel_filter',
    'model.model_utils.gaussian_filter': 'vit_ae_plus_plus_amd.model.model_utils.gaussian_filter',
    'model.model_utils.perceptual_loss': 'vit_ae_plus_plus_amd.model.model_utils.perceptual_loss',
    'utils': 'vit_ae_plus_plus_amd.utils',
    'utils.misc': 'vit_ae_plus_plus_amd.utils.misc',
    'utils.lr_sched': 'vit_ae_plus_plus_amd.utils.lr_sched',
    'utils.train_one_epoch': 'vit_ae_plus_plus_amd.utils.train_one_epoch',
    'utils.custom_loss': 'vit_ae_plus_plus_amd.utils.custom_loss',
    'utils.lr_decay': 'vit_ae_plus_plus_amd.utils.lr_decay',
    'utils.used_metrics': 'vit_ae_plus_plus_amd.utils.used_metrics',
    'utils.mixup': 'vit_ae_plus_plus_amd.utils.mixup',
    'post_training_utils': 'vit_ae_plus_plus_amd.post_training_utils',
    'post_training_utils.fine_tune_epoch': 'vit_ae_plus_plus_amd.post_training_utils.fine_tune_epoch',
    # the MoCo v3 baseline (other_baselines/mocov3/main_3d_moco_k_fold.py: `import other_baselines.mocov3.moco.builder` / `.optimizer`)
    'other_baselines': 'vit_ae_plus_plus_amd.other_baselines',
    'other_baselines.mocov3': 'vit_ae_plus_plus_amd.other_baselines.mocov3',
    'other_baselines.mocov3.moco': 'vit_ae_plus_plus_amd.other_baselines.mocov3.moco',
    'other_baselines.mocov3.moco.builder': 'vit_ae_plus_plus_amd.other_baselines.mocov3.moco.builder',
    'other_baselines.mocov3.moco.optimizer': 'vit_ae_plus_plus_amd.other_baselines.mocov3.moco.optimizer',
    # (the baseline's own copy of the encoder is model/vit.py without the contrastive class)
    'other_baselines.mocov3.moco.vit_3d': 'vit_ae_plus_plus_amd.model.vit',
    # its copy of the 3-D ResNet (keyword num_classes): the backbone of MoCo_ResNet, the script's default --arch
    'other_baselines.mocov3.moco.resent3d_base': 'vit_ae_plus_plus_amd.other_baselines.mocov3.moco.resent3d_base',
    # the supervised 3-D ResNet baseline; the pre-training scripts import get_all_feat_and_labels from train_3d_resnet
    'k_fold_training_scripts': 'vit_ae_plus_plus_amd.k_fold_training_scripts',
    'k_fold_training_scripts.resnet_3d': 'vit_ae_plus_plus_amd.k_fold_training_scripts.resnet_3d',
    'k_fold_training_scripts.train_3d_resnet': 'vit_ae_plus_plus_amd.k_fold_training_scripts.train_3d_resnet',
}


def install(force: bool = False):
    for alias, target in _ALIASES.items():
        if alias in sys.modules and not force and sys.modules[alias].__name__ != target:
            raise ImportError(f'{alias} is already imported from elsewhere ({sys.modules[alias]}); '
                              f'call install() before importing the reference packages or pass force=True')
        sys.modules[alias] = importlib.import_module(target)
